"""GPU suite (-m gpu): the ragged sweep encode — images of differing sizes, each at candidate rank triples of its own, in one call
(Context.encode_ragged_sweep, lrf_qmf_encode_ragged_sweep_rgb_u8) — against Context.encode_ragged called for every (image, triple)
alone, which tests/test_encode_ragged_gpu.py pins to the uniform encoder and the CPU oracle.  Everything is compared bitwise."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ragged_sweep_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
fam = lambda r: 0 if r <= 8 else (1 if r <= 16 else 2)


class Made:
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            from lrf_amd import _lib
            cls._made = (_lib.context(0), [W.content(j, H, Wd) for j, (H, Wd) in enumerate(W.SIZES)], W.interleaved(W.CANDS))
        return cls._made


def test_the_list_is_what_it_is_meant_to_be():
    from lrf_amd import _lib
    pairs = W.interleaved(W.CANDS)
    assert sorted(len(c) for c in W.CANDS) == [1, 2, 3, 5] and len(pairs) == 11
    assert all(a[0] != b[0] for a, b in zip(pairs, pairs[1:6]))  # interleaved: neighbours belong to different images
    assert {fam(t[0]) for t in W.CANDS[0]} == {0, 1, 2}                      # one image across the three rank families
    assert W.CANDS[2][0][1:] == W.CANDS[2][1][1:] and W.CANDS[2][0][0] != W.CANDS[2][1][0]  # two candidates share the chroma ranks
    for (H, Wd), cs in zip(W.SIZES, W.CANDS):                               # every rank within what qmf_ranks can give
        assert all(r <= min(d[4], 64) for t in cs for d, r in zip(_lib.plane_dims(H, Wd), t))
    assert [(H % 16 == 0 and Wd % 16 == 0, H % 2, Wd % 2) for H, Wd in W.SIZES] == [(True, 0, 0), (False, 0, 0), (False, 1, 1), (True, 0, 0)]


@pytest.mark.parametrize("k", [1, 10])
def test_every_candidate_equals_the_ragged_encoder_alone(k):
    ctx, imgs, pairs = Made.get()
    bad = W.differing(W.sweep(ctx, imgs, W.SIZES, pairs, k), W.alone(ctx, imgs, W.SIZES, pairs, k), pairs)
    assert not bad, bad


@pytest.mark.parametrize("k", [1, 10])
def test_per_image_signs_every_candidate_uses_the_leading_ones(k):
    ctx, imgs, pairs = Made.get()
    rng = np.random.default_rng(5)
    signs = []
    for i, cs in enumerate(W.CANDS):
        rmax = [max(t[ch] for t in cs) for ch in range(3)]
        signs.append(None if i == 1 else (rng.choice(np.array([-1, 1], dtype=np.int8), sum(rmax)), rmax))  # image 1 keeps the default signs
    want = W.alone(ctx, imgs, W.SIZES, pairs, k, signs)
    bad = W.differing(W.sweep(ctx, imgs, W.SIZES, pairs, k, signs), want, pairs)
    assert not bad, bad
    plain = W.alone(ctx, imgs, W.SIZES, pairs, k)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, plain)), "the signs changed nothing: the test shows nothing"


def test_candidates_in_image_order_and_one_image_alone():
    ctx, imgs, pairs = Made.get()
    ordered = [(i, t) for i, cs in enumerate(W.CANDS) for t in cs]
    assert not W.differing(W.sweep(ctx, imgs, W.SIZES, ordered, 10), W.alone(ctx, imgs, W.SIZES, ordered, 10), ordered)
    for i in range(len(W.SIZES)):
        one = [(0, t) for t in W.CANDS[i]]
        assert not W.differing(W.sweep(ctx, [imgs[i]], [W.SIZES[i]], one, 10), W.alone(ctx, [imgs[i]], [W.SIZES[i]], one, 10), one), i


@pytest.mark.parametrize("env", [dict(LRF_PERSIST="0"), dict(LRF_PERSIST="1"), dict(LRF_FAMILY_SPLIT_BLOCKS="1", LRF_BCDW32_MIN_BLOCKS="1"),
                                 dict(LRF_FAMILY_SPLIT_BLOCKS="1", LRF_BCDW16_MIN_BLOCKS="1", LRF_PERSIST="0")],
                         ids=["persist0", "persist1", "split_w32", "split_w16"])
def test_kernel_choices_in_a_child_process(env):
    """tests/_ragged_sweep_worker.py under the switches the ragged and sweep suites toggle: the persistent kernel off and at its test
    threshold (with a list large enough as one call to take it), every plane on the family of its own rank from one block on
    (the initialisations then cross families), the wave kernels from one block on"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_ragged_sweep_worker.py")], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "DONE" in r.stdout, r.stdout[-2000:]
    d = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert d["cands"] == 11 and d["nbad"] == 0 and d["ctx"] == "", d
    if env.get("LRF_PERSIST") == "1":
        assert d["big"] == 56 and d["blocks"] == 1152
        assert d["persist"] == 1, f"LRF_K_BCD_PERSIST launches: {d['persist']} (LRF_K_BCD regions: {d['bcd']})"


def test_c_entry_refuses_on_the_host_and_launches_nothing():
    from lrf_amd import _lib
    ctx = _lib.context(0)
    lib = _lib.load()
    H, Wd, r1, r2 = 64, 96, (7, 3, 3), (12, 6, 6)
    dims = _lib.plane_dims(H, Wd)
    nu = [sum(d[4] * r for d, r in zip(dims, t)) for t in (r1, r2)]
    nv = [64 * sum(t) for t in (r1, r2)]
    npx, ns = 3 * H * Wd, 12 + 6 + 6
    U = torch.full((2 * sum(nu),), 0x5A, dtype=torch.int8, device="cuda")
    V = torch.full((2 * sum(nv),), 0x5A, dtype=torch.int8, device="cuda")
    rgb = torch.randint(0, 256, (2 * npx,), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    sign = torch.ones((2 * ns,), dtype=torch.int8, device="cuda")
    ims_ok = [(H, Wd, 0, 0), (H, Wd, npx, -1)]
    cds_ok = [(0, r1, 0, 0), (1, r1, nu[0], nv[0]), (0, r2, 2 * nu[0], 2 * nv[0]), (1, r2, 2 * nu[0] + nu[1], 2 * nv[0] + nv[1])]

    def call(ims, cds, n=None, m=None, K=10, lo=-16, hi=15, u_len=U.numel(), v_len=V.numel(), rgb_len=rgb.numel(), sign_len=sign.numel(), u=U, v=V,
             src=rgb, sg=sign):
        idesc = (_lib.RaggedSweepImage * max(1, len(ims or [])))()
        for d, (h, w, ro, so) in zip(idesc, ims or []):
            d.H, d.W, d.rgb_off, d.sign_off = h, w, ro, so
        cdesc = (_lib.RaggedSweepCandidate * max(1, len(cds or [])))()
        for d, (i, r, uo, vo) in zip(cdesc, cds or []):
            d.image, d.u_off, d.v_off = i, uo, vo
            d.R[0], d.R[1], d.R[2] = r
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ctx.use_torch_stream()
        return lib.lrf_qmf_encode_ragged_sweep_rgb_u8(ctx._h, len(ims or []) if n is None else n, idesc if ims is not None else None,
                                                      len(cds or []) if m is None else m, cdesc if cds is not None else None, ptr(src), rgb_len, K, lo, hi,
                                                      ptr(sg), sign_len, ptr(u), u_len, ptr(v), v_len)

    im1 = lambda **kw: [ims_ok[0], tuple(kw.get(k, x) for k, x in zip(("H", "W", "rgb", "s"), ims_ok[1]))]
    cd3 = lambda **kw: cds_ok[:3] + [tuple(kw.get(k, x) for k, x in zip(("image", "R", "u", "v"), cds_ok[3]))]
    einval = {
        "u range": call(ims_ok, cds_ok, u_len=U.numel() - 1),
        "v range": call(ims_ok, cds_ok, v_len=V.numel() - 1),
        "rgb range": call(ims_ok, cds_ok, rgb_len=2 * npx - 1),
        "sign range": call(im1(s=2 * ns - ns + 1), cds_ok),
        "sign range at the image's largest ranks": call(ims_ok, cds_ok, sign_len=ns - 1),
        "u offset past the end": call(ims_ok, cd3(u=2 * nu[0] + nu[1] + 1)),
        "v offset past the end": call(ims_ok, cd3(v=2 * nv[0] + nv[1] + 1)),
        "rgb offset past the end": call(im1(rgb=npx + 1), cds_ok),
        "negative u": call(ims_ok, cd3(u=-1)),
        "negative v": call(ims_ok, cd3(v=-1)),
        "negative rgb": call(im1(rgb=-16), cds_ok),
        "sign offset -2": call(im1(s=-2), cds_ok),
        "offset near 2^63": call(ims_ok, cd3(u=2 ** 63 - 1)),
        "U ranges of two candidates overlap": call(ims_ok, cd3(u=2 * nu[0] - 1)),
        "V ranges of two candidates overlap": call(ims_ok, cd3(v=0)),
        "a candidate naming no image": call(ims_ok, cd3(image=2)),
        "a candidate naming image -1": call(ims_ok, cd3(image=-1)),
        "an image with no candidate": call(ims_ok, [(0, r, uo, vo) for _, r, uo, vo in cds_ok]),
        "fewer candidates than images": call(ims_ok, cds_ok[:1]),
        "rank 0": call(ims_ok, cd3(R=(7, 0, 3))),
        "n = 0": call(ims_ok, cds_ok, n=0),
        "n = 65536": call(ims_ok, cds_ok, n=65536, m=65536),
        "m = 2^20 + 1": call(ims_ok, cds_ok, m=2 ** 20 + 1),
        "no size": call(im1(H=0), cds_ok),
        "1x1": call(im1(H=1, W=1), cds_ok),
        "bounds outside int8": call(ims_ok, cds_ok, hi=128),
        "lo > hi": call(ims_ok, cds_ok, lo=3, hi=2),
        "NULL images": call(None, cds_ok, n=2),
        "NULL candidates": call(ims_ok, None, m=4),
        "NULL rgb": call(ims_ok, cds_ok, src=None),
        "NULL U": call(ims_ok, cds_ok, u=None),
        "NULL V": call(ims_ok, cds_ok, v=None),
    }
    assert all(rc == -1 for rc in einval.values()), einval
    enotsup = {
        "rank 33": call(ims_ok, cd3(R=(33, 3, 3))),
        "rank 65": call(ims_ok, cd3(R=(65, 3, 3))),
        "K = 0": call(ims_ok, cds_ok, K=0),
        "an image of 2^31 / 3 pixels or more": call(im1(H=30000, W=30000), cds_ok),
    }
    assert all(rc == -2 for rc in enotsup.values()), enotsup
    torch.cuda.synchronize()
    assert bool((U == 0x5A).all()) and bool((V == 0x5A).all()), "a refused call wrote to its output"
    assert call(ims_ok, cds_ok) == 0  # and the same call with the arguments right runs
    assert call(ims_ok, cds_ok, sg=None, sign_len=0) == 0  # a NULL sign: default signs for every image, whatever its sign_off
    torch.cuda.synchronize()
    assert not bool((U == 0x5A).any()) and not bool((V == 0x5A).all())
    flat = rgb
    for ims, cds in (([(H, Wd, npx + 1)], [(0, r1)]), ([(H, Wd, 0)], [(0, (7, 3, 33))]), ([(H, Wd, 0)], [(1, r1)]), ([(H, Wd, 0), (H, Wd, npx)], [(0, r1), (0, r2)]),
                     ([], []), ([(H, Wd, 0)], [])):
        with pytest.raises(ValueError):
            ctx.encode_ragged_sweep(flat, ims, cds, 10, -16, 15)
    with pytest.raises(TypeError):
        ctx.encode_ragged_sweep(flat.float(), [(H, Wd, 0)], [(0, r1)], 10, -16, 15)
