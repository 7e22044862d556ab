"""CPU suite: the gates of the geometry sweep (tests/geometry_cases.py).  The definition written there with torch's CPU operators
is compared bit for bit with the CPU oracle over every grid the GPU module (tests/test_geometry_gpu.py) uses, and with the
reference's recorded pixels; the test data is shown to be what the GPU module needs (pixels clear of the clamp, so that a chroma row
taken one off, a crop offset off by one or another nearest index would change the expected bytes: each such mistake is made on
purpose here and must change at least a fifth of them); and the grids are shown, by a rule restated by hand from the comments of
decode_plan and lrf_qmf_planes_from_rgb_u8, to reach every decode launch group and every planes body."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import geometry_cases as G
from conftest import QMF_CASES, Case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lrf_amd", "csrc")
SF_CASES = ["sf_quarter_q10", "sf_444_r5", "sf_mixed_odd_q12", "sf_nopatch_q8"]
SATURATED_MAX = 0.05   # conditions on the inputs, not measurements of the kernels: the data measures 0.02 and 0.37 against them
MUTANT_MIN = 0.20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_planes(got, want, what):
    for c in range(3):
        assert got[c].shape == want[c].shape, (what, c, got[c].shape, want[c].shape)
        assert np.array_equal(_bits(got[c]), _bits(want[c])), (what, "plane", c)


# ---- the oracle against the definition ----------------------------------------------------------------------------------------
def test_oracle_planes_equal_the_definition_on_every_residue(oracle):
    for H, W in G.RESIDUES + G.WIDE:
        _same_planes(oracle.rgb_to_planes(G.image(H, W).numpy()), G.planes(H, W), (H, W))


@pytest.mark.parametrize("sf", G.SCALE_FACTORS, ids=[f"{a:.3g}x{b:.3g}" for a, b in G.SCALE_FACTORS])
def test_oracle_anyshape_equals_the_definition(sf, oracle):
    """planes and decode for every scale factor x patch setting x size of ANY"""
    cases = G.any_cases(sf)
    assert len(cases) >= 60 and {c[2] for c in cases} >= {(8, 8), (4, 4), None}
    for H, W, ps, chroma in cases:
        img = G.image(H, W)
        _same_planes(oracle.anyshape_matrices(img.numpy(), ps, chroma), G.ref_planes(img, sf, ps), (H, W, sf, ps))
        f6 = G.midrange_factors(np.random.default_rng([H, W, 9]), H, W, G.ANY_RANKS, ps, chroma)
        want = G.ref_decode(f6, H, W, ps, chroma)
        got = oracle.qmf_anyshape_decode(list(zip(f6[0::2], f6[1::2])), H, W, ps, chroma)
        assert np.array_equal(got, want), (H, W, sf, ps)


@pytest.mark.parametrize("ranks", G.DECODE_TRIPLES, ids=str)
def test_oracle_decode_equals_the_definition_on_every_residue(ranks, oracle):
    sizes = G.RESIDUES + (G.WIDE if ranks in G.WIDE_TRIPLES else [])
    for H, W in sizes:
        f6 = G.factors(H, W, ranks)
        assert np.array_equal(oracle.planes_to_rgb(f6[0::2], f6[1::2], H, W), G.decoded(H, W, ranks)), (H, W, ranks)


def test_default_scale_through_the_anyshape_oracle_too(oracle):
    """the any-shape oracle at the default settings is the 8 x 8 oracle: both pins agree with each other on the diagonal"""
    for H, W in G.DIAGONAL:
        f6 = G.factors(H, W, (7, 3, 3))
        assert np.array_equal(oracle.qmf_anyshape_decode(list(zip(f6[0::2], f6[1::2])), H, W, (8, 8)), G.decoded(H, W, (7, 3, 3))), (H, W)
        _same_planes(oracle.anyshape_matrices(G.image(H, W).numpy(), (8, 8)), G.planes(H, W), (H, W))


def test_colour_products_are_torchs_einsum_within_the_roundings_of_a_three_term_sum():
    """geometry_cases.colour_product against torch.einsum with the same matrices: any order of an fp32 three-term sum of values
    below 256, fused or not, stays within three roundings of the exact value, the offset adds a fourth: two such results differ by
    at most 2 * 4 * 2^-17 = 2^-14.  (Whether they are equal bit for bit depends on the host's BLAS: printed, not asserted.)"""
    worst_p = worst_d = 0.0
    for H, W in G.RESIDUES[::5]:
        a, b = G.planes(H, W), G.ref_planes(G.image(H, W), einsum=True)
        worst_p = max(worst_p, max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b)))
        f6 = G.factors(H, W, (7, 3, 3))
        a, b = G.ref_decode(f6, H, W, as_float=True), G.ref_decode(f6, H, W, einsum=True, as_float=True)
        assert np.abs(a).max() < 512
        worst_d = max(worst_d, float(np.abs(a.astype(np.float64) - b).max()))
    print(f"colour_product against torch.einsum: planes {worst_p:.3g}, decoded float image {worst_d:.3g}")
    assert worst_p <= 2.0 ** -14 and worst_d <= 2.0 ** -13  # (the decoded image's values reach 512: one more bit)


# ---- the reference's recorded pixels --------------------------------------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", QMF_CASES + SF_CASES)
def test_definition_decodes_the_reference_streams_to_the_reference_pixels(name):
    c = Case(name)
    kw = c.kwargs
    assert kw.get("color_space", "YCbCr") == "YCbCr"
    H, W = c.image.shape[-2:]
    ps = tuple(kw.get("patch_size", (8, 8))) if kw.get("patch", True) else None
    sf = tuple(kw.get("scale_factor", (0.5, 0.5)))
    f6 = [np.asarray(f).reshape(-1, f.shape[-1]) for f in c.ref_factors()]
    assert _sha(G.ref_decode(f6, H, W, ps, G.chroma_of(H, W, sf))) == c.decoded_sha256


# ---- conditions on the inputs ---------------------------------------------------------------------------------------------------
def _grid():
    return [(H, W, t) for t in G.DECODE_TRIPLES for H, W in G.RESIDUES] + [(H, W, t) for t in G.WIDE_TRIPLES for H, W in G.WIDE]


def test_expected_images_stay_clear_of_the_clamp():
    worst = max((G.saturated(G.decoded(H, W, t, k)), (H, W, t, k)) for H, W, t in _grid() for k in (0, 1))
    print(f"largest share of bytes at 0 or 255: {worst[0]:.4f} at {worst[1]}")
    assert worst[0] <= SATURATED_MAX, worst


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_each_mistake_would_change_the_expected_bytes(mutant):
    least, applied = (1.0, None), 0
    for H, W, t in _grid():
        if not G.mutant_applies(mutant, H, W):
            continue
        applied += 1
        changed = float(np.mean(G.ref_decode(G.factors(H, W, t), H, W, mutant=mutant) != G.decoded(H, W, t)))
        least = min(least, (changed, (H, W, t)))
    print(f"{mutant}: smallest share of changed bytes {least[0]:.4f} at {least[1]} over {applied} images")
    # top: chroma rows are padded unless (H // 2) % 8 == 0, i.e. H % 16 in {0, 1}; left: luma columns unless W % 8 == 0
    want = {"top": 14 * 16, "left": 14 * 16, "nearest": 256}[mutant] * len(G.DECODE_TRIPLES) + {"top": 14, "left": 14, "nearest": 16}[mutant] * len(G.WIDE_TRIPLES)
    assert applied == want, (applied, want)
    assert least[0] >= MUTANT_MIN, least


def test_anyshape_expected_images_stay_clear_of_the_clamp():
    worst = (0.0, ())
    for sf in G.SCALE_FACTORS:
        for H, W, ps, chroma in G.any_cases(sf)[::7]:
            f6 = G.midrange_factors(np.random.default_rng([H, W, 9]), H, W, G.ANY_RANKS, ps, chroma)
            worst = max(worst, (G.saturated(G.ref_decode(f6, H, W, ps, chroma)), (H, W, sf, ps)))
    assert worst[0] <= SATURATED_MAX, worst


# ---- coverage: which kernel each size reaches, by the hand-restated rule ---------------------------------------------------------
def test_the_grids_reach_every_decode_group_and_class():
    groups = {G.decode_group(H, W, t) for H, W in G.RESIDUES for t in G.TRIPLES}
    assert {(G.DEC_TILE16, c) for c in (0, 1, 2, 4)} <= groups       # (32, 32): the one 16-aligned size of RESIDUES
    assert {(G.DEC_STRIP, c) for c in (0, 1, 2, 4)} <= groups
    assert (G.DEC_R8, 0) in groups and (G.DEC_ANY, 0) in groups
    # class 3 (luma <= 16 with chroma 9..16) has no triple in TRIPLES — (16,8,8) is of class 2 — so the decode tests add CLASS3
    assert (G.DEC_TILE16, 3) not in groups and (G.DEC_STRIP, 3) not in groups
    groups |= {G.decode_group(H, W, G.CLASS3) for H, W in G.RESIDUES}
    assert {(k, c) for k in (G.DEC_TILE16, G.DEC_STRIP) for c in range(5)} <= groups
    assert [G.decode_group(32, 32, t)[1] for t in G.DECODE_TRIPLES[:6] + [G.CLASS3]] == [0, 0, 1, 2, 4, 4, 3]
    per_kind = {k: sum(G.decode_group(H, W, (7, 3, 3))[0] == k for H, W in G.RESIDUES) for k in range(4)}
    # strip: W even, an even luma left crop, chroma columns four-aligned under it — W % 16 in {0, 12} (left crops 0 / 0 and 2 / 1)
    assert per_kind == {G.DEC_TILE16: 1, G.DEC_STRIP: 31, G.DEC_R8: 224, G.DEC_ANY: 0}, per_kind
    assert {G.decode_group(H, W, (64, 64, 64))[0] for H, W in G.RESIDUES} == {G.DEC_ANY}
    assert {G.decode_group(H, W, t)[0] for H, W in G.WIDE for t in G.WIDE_TRIPLES} >= {G.DEC_TILE16, G.DEC_STRIP, G.DEC_R8, G.DEC_ANY}


def test_the_grids_reach_every_planes_body():
    bodies = [G.planes_body(H, W) for H, W in G.RESIDUES]
    assert [bodies.count(b) for b in range(5)] == [1, 63, 64, 64, 64]
    # WIDE's H and W are of one parity (5 j mod 16 and j): the 16-aligned body and the windows <2,2> and <3,3> with per_strip > 1
    assert {G.planes_body(H, W) for H, W in G.WIDE} == {G.ENC_TILE16, G.ENC_STRIP22, G.ENC_STRIP33}
    assert {G.planes_body(H, W, aligned8=False) for H, W in G.DIAGONAL} == {G.ENC_STRIP22, G.ENC_STRIP33}
    assert G.planes_body(32, 32, aligned8=False) == G.ENC_STRIP22 and G.planes_body(48, 48, aligned8=False) == G.ENC_STRIP22


def test_wide_spans_more_than_one_column_group():
    assert all(G.per_strip(W) > 1 for _, W in G.WIDE) and all(G.per_strip(W) == 1 for _, W in G.RESIDUES)
    assert sorted(H % 16 for H, _ in G.WIDE) == list(range(16)) and sorted(W % 16 for _, W in G.WIDE) == list(range(16))
    assert sorted((H % 16, W % 16) for H, W in G.RESIDUES) == [(i, j) for i in range(16) for j in range(16)]


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("geometry_plan")
    libs = []
    for shim in ("decode_ragged_plan_shim.cpp", "encode_ragged_plan_shim.cpp"):
        so = str(d / (shim[:-4] + ".so"))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(CSRC, "lrf_plan.cpp"),
                               os.path.join(HERE, shim)])
        libs.append(ctypes.CDLL(so))
    return libs


def test_hand_rule_is_the_librarys_plan_over_the_grids(shims):
    import test_encode_ragged_plan as ERP
    dec, enc = shims
    for H, W in G.RESIDUES + G.WIDE:
        for t in G.DECODE_TRIPLES + [(12, 12, 12), (8, 16, 16), (33, 4, 4), (5, 17, 2)]:
            for aligned8 in (True, False):
                got = dec.lrf_test_decode_plan(H, W, t[0], t[1], t[2], aligned8, False)
                assert got >= 0 and divmod(got, 8) == G.decode_group(H, W, t, aligned8), (H, W, t, aligned8)
    sizes = G.RESIDUES + G.WIDE
    for aligned8 in (True, False):
        ims = ERP.make([(H, W, (3, 2, 2)) for H, W in sizes])
        for im in ims:
            im["aligned8"] = aligned8
        p = ERP.plan(enc, ims)
        assert not p["too_many"]
        for (H, W), d in zip(sizes, p["descs"]):
            assert d["body"] == G.planes_body(H, W, aligned8), (H, W, aligned8)
            if d["body"] == G.ENC_TILE16:
                assert d["per_strip"] == G.per_strip(W), (H, W)
