"""CPU suite: the launch plan of a call of the 64-column path (plan_bcd, lrf_amd/csrc/lrf_plan.cpp) — which U-update kernel
iterates which run of planes, whether one persistent launch k_bcd_p<F16, NP32, FIRST> takes the iterations, how the rank
families share streams.  The plan source needs no device: it is built here with g++ together with tests/bcd_plan_shim.cpp and
called through ctypes, with planes made by the library's own add_plane.

Expected values never come from the plan:
  * the persistent launch of every case that tests/test_persist_at_size.py runs on a GPU — the tables at the top of
    tests/_persist_at_size_worker.py record, per case, the launches counted there and the instantiation that makes them;
  * the per-family rules of small calls from the thresholds of lrf_plan.h (1024 / 1024 / 128 blocks, 2304 / 3584 blocks for the
    persistent launch) and the two bounds (R - 1) 64 mx^3 < 2^24 and 64 mx^2 <= 32767, worked out by hand in each test.
The sweep cases of that worker stay with the GPU test: the sweep's plane order is made inside its entry point, behind a context."""
import ctypes
import os
import subprocess

import pytest

import _persist_at_size_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
WG8, WG16, MID, K_W, K_W16, K_W32, K_W32F = range(7)   # enum BcdKernel
NONE, INIT, CALL = range(3)                            # enum FamStreams
FIRST_W0, FIRST_U0 = 1, 2                              # first_mode
WAVE_OF_FAM = (K_W, K_W16, K_W32)
MIN_BLOCKS_OF_FAM = (1024, 1024, 128)                  # LRF_BCDW_MIN_BLOCKS, LRF_BCDW16_MIN_BLOCKS, LRF_BCDW32_MIN_BLOCKS
HEAD = ("persist", "f16", "np32", "first", "streams", "mixed", "split", "rp", "rmax", "nblocks")
RUN = ("plane0", "nplanes", "block0", "nblocks", "rmin", "rmax", "fam", "pitch", "exact_int", "first_k", "first_arg", "later_k", "later_arg",
       "nbase", "any_native")
SETTINGS = ("persist", "family_split_blocks", "bcdw16_min_blocks", "bcdw32_min_blocks", "bcd_wg", "no_family_split", "no_family_streams",
            "no_bcdw32", "generic_gs", "no_persist_first", "no_init_fork", "persist_arch")
DEFAULTS = dict(persist=-1, family_split_blocks=-1, bcdw16_min_blocks=-1, bcdw32_min_blocks=-1, persist_arch=1)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bcd_plan") / "libbcd_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(CSRC, "lrf_plan.cpp"), os.path.join(HERE, "bcd_plan_shim.cpp")])
    return ctypes.CDLL(so)


def plan(lib, planes, K=10, bounds=W.D, first_mode=FIRST_W0, **settings):
    """planes: [(M, R)] in table order -> (head dict, [run dict])"""
    n = len(planes)
    M = (ctypes.c_int * n)(*[p[0] for p in planes])
    R = (ctypes.c_int * n)(*[p[1] for p in planes])
    s = dict(DEFAULTS, **settings)
    sv = (ctypes.c_long * len(SETTINGS))(*[int(s.get(k, 0)) for k in SETTINGS])
    head = (ctypes.c_int * len(HEAD))()
    runs = (ctypes.c_int * (len(RUN) * 8))()
    nruns = lib.lrf_test_plan_bcd(n, M, R, K, bounds[0], bounds[1], first_mode, 0, sv, head, runs, 8)
    assert 1 <= nruns <= 8
    return dict(zip(HEAD, head)), [dict(zip(RUN, runs[j * len(RUN):(j + 1) * len(RUN)])) for j in range(nruns)]


def image_planes(B, H, W_, ranks):
    """the table of the fused encode (encode_rgb_prepare): all Y planes, then Cb, then Cr; M by plane_dims' arithmetic"""
    def M(c):
        h, w = (H // 2, W_ // 2) if c else (H, W_)
        return ((h + 7) // 8) * ((w + 7) // 8)
    return [(M(c), ranks[c]) for c in range(3) for _ in range(B)]


def check_recorded(head, K, path, inst):
    """path = (persistent launches, LRF_K_BCD regions) as counted on a GPU; inst the k_bcd_p instantiation or None"""
    assert head["persist"] == path[0]
    regions = 0 if head["first"] else (1 if head["persist"] else K)
    assert regions == path[1]
    if inst is None:
        assert not head["persist"]
    else:
        assert "<%s,%d,%s>" % ("true" if head["f16"] else "false", head["np32"], "true" if head["first"] else "false") == inst
    assert head["streams"] == (INIT if head["persist"] else CALL)


@pytest.mark.parametrize("ranks, bounds, K, path, inst", W.BATCH_CASES, ids=[W.case_name(*c[:3]) for c in W.BATCH_CASES])
def test_production_batch(lib, ranks, bounds, K, path, inst):
    head, _ = plan(lib, image_planes(*W.BATCH, ranks), K, bounds)
    assert head["nblocks"] == 256 * 24  # 512x768: 16 + 4 + 4 blocks an image
    check_recorded(head, K, path, inst)


@pytest.mark.parametrize("ranks, below, at", W.THRESHOLD_CASES, ids=[str(c[0]) for c in W.THRESHOLD_CASES])
def test_thresholds_straddled(lib, ranks, below, at):
    """96 x 24 = 2304 = LRF_PERSIST_MIN_BLOCKS_ONE_FAMILY; 149 x 24 = 3576 < LRF_PERSIST_MIN_BLOCKS = 3584 <= 150 x 24"""
    lo, _ = plan(lib, image_planes(below, 512, 768, ranks))
    hi, _ = plan(lib, image_planes(at, 512, 768, ranks))
    assert not lo["persist"] and lo["streams"] == CALL
    assert hi["persist"] and hi["first"] and hi["streams"] == INIT


@pytest.mark.parametrize("shape, case", [(s, c) for s, cases in W.SHAPE_CASES for c in cases],
                         ids=[f"{s} {W.case_name(*c[:3])}" for s, cases in W.SHAPE_CASES for c in cases])
def test_other_geometries(lib, shape, case):
    ranks, bounds, K, path, inst = case
    head, _ = plan(lib, image_planes(*shape, ranks), K, bounds)
    check_recorded(head, K, path, inst)


@pytest.mark.parametrize("kind, M, R, K", [("bcd",) + c for c in W.CALLER_BCD] + [("decompose",) + c for c in W.CALLER_DECOMPOSE])
def test_uniform_tables_of_a_caller(lib, kind, M, R, K):
    """Context.bcd (the caller's U0: first_mode 2, never forked) and Context.decompose on 160 equal matrices"""
    head, runs = plan(lib, [(M, R)] * W.CALLER_B, K, W.D, FIRST_U0 if kind == "bcd" else FIRST_W0)
    path, inst = W.caller_path(kind, R), W.caller_inst(kind, R)
    assert head["persist"] == path[0] and (0 if head["first"] else 1) == path[1]
    assert "<%s,%d,%s>" % ("true" if head["f16"] else "false", head["np32"], "true" if head["first"] else "false") == inst
    assert head["streams"] == (NONE if kind == "bcd" else INIT)
    assert len(runs) == 1


def kernels(runs):
    return [((r["first_k"], r["first_arg"]), (r["later_k"], r["later_arg"])) for r in runs]


def test_rank8_run_flips_at_1024_blocks(lib):
    """LRF_BCDW_MIN_BLOCKS: below it the workgroup kernel k_bcd<., 8>, from it on k_bcd_w, first and later iterations alike"""
    assert kernels(plan(lib, [(384, 8)] * 1023)[1]) == [((WG8, 0), (WG8, 0))]
    assert kernels(plan(lib, [(384, 8)] * 1024)[1]) == [((K_W, 0), (K_W, 0))]


def test_rank16_run_outside_the_exact_integer_bound(lib):
    """(-32, 31): 15 * 64 * 32^3 = 31457280 >= 2^24, so iterations >= 2 stay on k_bcd<0, 16>; the first iteration does not
    depend on that bound: k_bcd_w16<1>.  Inside the bound ((-16, 15): 15 * 64 * 16^3 < 2^24) both are k_bcd_w16."""
    for n in (1024, 1500):
        _, runs = plan(lib, [(384, 16)] * n, bounds=(-32, 31))
        assert kernels(runs) == [((K_W16, 0), (WG16, 0))] and not runs[0]["exact_int"]
    _, runs = plan(lib, [(384, 16)] * 1024)
    assert kernels(runs) == [((K_W16, 0), (K_W16, 0))] and runs[0]["exact_int"]
    assert kernels(plan(lib, [(384, 16)] * 1023)[1]) == [((WG16, 0), (WG16, 0))]


def test_uniform_rank20_run_flips_at_128_blocks(lib):
    """LRF_BCDW32_MIN_BLOCKS: k_bcd_mid below; from it on k_bcd_w32f<20> for the first iteration and k_bcd_w32<10> for the later
    ones (19 * 64 * 16^3 < 2^24 and 64 * 16^2 = 16384 <= 32767).  (-22, 22): 64 * 22^2 = 30976 still fits int16 and 19 * 64 *
    22^3 < 2^24; (-23, 23): 64 * 23^2 = 33856 does not fit: k_bcd_mid for the later iterations."""
    assert kernels(plan(lib, [(384, 20)] * 127)[1]) == [((MID, 0), (MID, 0))]
    assert kernels(plan(lib, [(384, 20)] * 128)[1]) == [((K_W32F, 20), (K_W32, 10))]
    assert kernels(plan(lib, [(384, 20)] * 128, bounds=(-22, 22))[1]) == [((K_W32F, 20), (K_W32, 10))]
    assert kernels(plan(lib, [(384, 20)] * 128, bounds=(-23, 23))[1]) == [((K_W32F, 20), (MID, 0))]


def test_rank_17_to_32_run_of_two_ranks(lib):
    """256 blocks with a rank above 16: the call splits by family, both ranks fall into family 2 — one run; k_bcd_w32f is
    instantiated per rank, so the first iteration is k_bcd_mid; k_bcd_w32<10> (pairs of the larger rank) takes the later ones"""
    head, runs = plan(lib, [(384, 20)] * 128 + [(384, 18)] * 128)
    assert head["split"] and kernels(runs) == [((MID, 0), (K_W32, 10))]


@pytest.mark.parametrize("R, n, later", [(8, 1024, (K_W, 0)), (12, 1024, (K_W16, 0)), (20, 128, (K_W32, 10)), (12, 2400, (K_W16, 0)), (20, 2400, (K_W32, 10))])
def test_callers_u0_first_iteration(lib, R, n, later):
    """first_mode 2: the wave kernels of ranks above 8 have no body that reads a caller's fp32 U0; k_bcd_w<2> has.  Never inside
    the persistent launch, never forked."""
    head, runs = plan(lib, [(384, R)] * n, first_mode=FIRST_U0)
    first = {8: (K_W, 0), 12: (WG16, 0), 20: (MID, 0)}[R]
    assert kernels(runs) == [(first, later)]
    assert head["persist"] == (n >= 2304) and not head["first"] and head["streams"] == NONE


def test_persist_switch_and_device(lib):
    """LRF_PERSIST=0: never; =1: from LRF_BCDW_MIN_BLOCKS blocks (43 x 24 = 1032 >= 1024 > 42 x 24); another device: never"""
    big = image_planes(256, 512, 768, (7, 3, 3))
    assert plan(lib, big)[0]["persist"]
    assert not plan(lib, big, persist=0)[0]["persist"]
    assert not plan(lib, big, persist_arch=0)[0]["persist"]
    assert plan(lib, image_planes(43, 512, 768, (7, 3, 3)), persist=1)[0]["persist"]
    assert not plan(lib, image_planes(42, 512, 768, (7, 3, 3)), persist=1)[0]["persist"]
    assert not plan(lib, image_planes(43, 512, 768, (7, 3, 3)))[0]["persist"]


GRID_RANKS = [(1, 1, 1), (4, 2, 2), (7, 3, 3), (8, 8, 8), (9, 4, 4), (12, 12, 12), (16, 8, 8), (16, 16, 16), (17, 8, 8), (18, 17, 17), (20, 10, 10),
              (20, 17, 17), (24, 12, 6), (26, 13, 13), (32, 16, 16), (32, 32, 32)]
GRID_BOUNDS = sorted({tuple(c[1]) for c in W.BATCH_CASES})


@pytest.mark.parametrize("bounds", GRID_BOUNDS, ids=str)
def test_persistent_plan_agrees_with_the_family_kernels(lib, bounds):
    """k_bcd_p runs the bodies of the families' wave kernels, so a persistent plan is only right where those kernels are: over 1..300
    images of 512x768, whenever the plan is persistent every run sits on its own family with exact-integer numbers above rank 8,
    and its later-iteration kernel is its family's wave kernel, with the launch's pair count at ranks 17..32.  One exception
    is left to the run's size, not its numbers: a run below its own family's block threshold (the two chroma runs of (24,12,6)
    from 150 to 255 images: 600..1020 blocks each) names the workgroup kernel for later iterations, which a persistent plan
    never launches; the thresholds of the persistent launch count the call's blocks, not a run's."""
    for ranks in GRID_RANKS:
        for B in range(1, 301):
            head, runs = plan(lib, image_planes(B, 512, 768, ranks), 10, bounds)
            if not head["persist"]:
                continue
            assert head["nblocks"] >= (2304 if len(runs) == 1 else 3584), (ranks, B)
            mx = max(abs(bounds[0]), abs(bounds[1]))
            for r in runs:
                fam = r["fam"]
                assert fam == (0 if r["rmax"] <= 8 else 1 if r["rmax"] <= 16 else 2) == (0 if r["rmin"] <= 8 else 1 if r["rmin"] <= 16 else 2), (ranks, B)
                assert fam == 0 or ((r["rmax"] - 1) * 64 * mx ** 3 < 2 ** 24 and r["exact_int"] and not r["any_native"]), (ranks, B)
                assert fam < 2 or 64 * mx * mx <= 32767, (ranks, B)
                if r["nblocks"] >= MIN_BLOCKS_OF_FAM[fam]:
                    assert (r["later_k"], r["later_arg"]) == (WAVE_OF_FAM[fam], head["np32"] if fam == 2 else 0), (ranks, B, r)
                else:
                    assert fam < 2 and len(runs) == 3, (ranks, B, r)
            assert head["f16"] == any(r["fam"] > 0 for r in runs) and head["first"] == (head["np32"] == 0), (ranks, B)
