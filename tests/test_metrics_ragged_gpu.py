"""GPU suite (-m gpu): squared error and SSIM of pairs that differ in size in one call (lrf_image_metrics_ragged_u8,
Context.metrics_ragged, lrf_amd.image_metrics_ragged).  The contract is "the bits of the uniform entry": pair i must give what
image_metrics_batch(a_i[None], b_i[None]) gives, compared as int64 views, NaN included; the squared error is an exact integer;
the host definition lrf_amd.metrics.ssim is met within the bar the uniform kernel carries (tests/metrics_cases.py: 1e-9).

Sizes: one tile (7x7, 7x70, 30x7, 30x70: the last window position of a tile of 24 x 64), one position into the next tile each
way (31x71), two whole tiles (54x134), one into the third (55x135), and 64x64 / 33x47.  The images start at offsets that are odd,
multiples of 4 and multiples of 16, so that with W they meet every load width."""
import ctypes
import math

import numpy as np
import pytest
import torch

from metrics_cases import SSIM_BAR

pytestmark = pytest.mark.gpu
SIZES = [(7, 7), (7, 70), (30, 7), (30, 70), (31, 71), (54, 134), (55, 135), (64, 64), (33, 47)]
# (size, where a starts, where b starts): an odd offset (1), a multiple of 4 but not of 16 (4), a multiple of 16 (16).  Only W = 64
# is a multiple of 4, so 64x64 comes twice: at multiples of 16 (16-byte loads) and at multiples of 4 (4-byte loads)
SPECS = list(zip(SIZES, [1, 4, 16, 1, 4, 16, 1, 16, 4], [4, 16, 1, 1, 4, 16, 16, 16, 1])) + [((64, 64), 4, 4)]
SHARE, CONST = len(SPECS), len(SPECS) + 1  # pair SHARE reads the a image of pair 5; pairs CONST, CONST + 1 a constant a image


def _place(end, align):
    """the first offset >= end of the alignment class `align`"""
    off = -(-end // align) * align
    if align == 1 and off % 2 == 0:
        off += 1
    if align == 4 and off % 16 == 0:
        off += 4
    return off


class Made:
    """the pairs, their flat buffers and the per-pair references: made once, left unchanged"""
    _made = None

    @classmethod
    def get(cls):
        if cls._made is None:
            import lrf_amd
            from lrf_amd import _lib
            ctx = _lib.context(0)
            rng = np.random.default_rng(5)
            imgs_a, imgs_b = [], []
            for (H, W), _, _ in SPECS:
                a = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
                imgs_a.append(a)
                imgs_b.append(np.clip(a.astype(int) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8))
            imgs_a.append(imgs_a[5])
            imgs_b.append(rng.integers(0, 256, imgs_a[5].shape, dtype=np.uint8))
            const = np.full((3, 20, 33), 77, np.uint8)  # a constant a: data_range 0
            imgs_a += [const, const]
            imgs_b += [np.full((3, 20, 33), 80, np.uint8), rng.integers(0, 256, const.shape, dtype=np.uint8)]
            aligns = [(x, y) for _, x, y in SPECS] + [(None, 4), (1, 16), (None, 1)]  # (None: the a image of an earlier pair)
            a_off, b_off, na, nb = [], [], 0, 0
            for i, (a, (xa, xb)) in enumerate(zip(imgs_a, aligns)):
                if xa is None:
                    a_off.append(a_off[5] if i == SHARE else a_off[-1])
                else:
                    a_off.append(_place(na, xa))
                    na = a_off[-1] + a.size
                b_off.append(_place(nb, xb))
                nb = b_off[-1] + a.size
            A, B = np.full((na + 5,), 0xEE, np.uint8), np.full((nb + 5,), 0xEE, np.uint8)
            for a, b, oa, ob in zip(imgs_a, imgs_b, a_off, b_off):
                A[oa:oa + a.size] = a.reshape(-1)
                B[ob:ob + b.size] = b.reshape(-1)
            pairs = [(a.shape[1], a.shape[2], oa, ob) for a, oa, ob in zip(imgs_a, a_off, b_off)]
            ta, tb = [torch.from_numpy(a) for a in imgs_a], [torch.from_numpy(b) for b in imgs_b]
            ref = [lrf_amd.image_metrics_batch(x.cuda()[None], y.cuda()[None]) for x, y in zip(ta, tb)]
            ref_ssim = torch.cat([r["ssim"] for r in ref]).cpu()
            ref_sse = torch.cat([r["sse"] for r in ref]).cpu()
            ref_psnr = torch.cat([r["psnr"] for r in ref]).cpu()
            cls._made = (ctx, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), pairs, ta, tb, ref_sse, ref_ssim, ref_psnr)
        return cls._made


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64).tolist()


def test_the_offsets_meet_every_load_width():
    ctx, A, B, pairs, *_ = Made.get()
    width = lambda H, W, oa, ob: next(v for v in (16, 4, 1) if ((A.data_ptr() + oa) | (B.data_ptr() + ob) | W) % v == 0)
    assert {width(*p) for p in pairs} == {16, 4, 1}
    assert {p[2] % 2 for p in pairs} == {0, 1} and any(p[2] % 16 == 0 for p in pairs) and any(p[2] % 4 == 0 and p[2] % 16 for p in pairs)
    assert pairs[SHARE][2] == pairs[5][2] and pairs[CONST + 1][2] == pairs[CONST][2]  # shared a images


def test_every_pair_has_the_bits_of_the_uniform_entry():
    ctx, A, B, pairs, ta, tb, ref_sse, ref_ssim, _ = Made.get()
    sse, ssim = ctx.metrics_ragged(A, B, pairs, 3)
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.is_cuda and tuple(ssim.shape) == (len(pairs),)
    exact = [int(((x.long() - y.long()) ** 2).sum()) for x, y in zip(ta, tb)]
    print("sse", sse.tolist(), "ssim", ssim.tolist(), "uniform", ref_ssim.tolist())
    assert sse.tolist() == exact == ref_sse.tolist()
    assert bits(ssim) == bits(ref_ssim)
    assert math.isnan(ssim[CONST].item()) and not math.isnan(ssim[0].item())  # constant a against constant b: NaN, as the host gives


def test_ssim_meets_the_host_definition():
    from lrf_amd import metrics
    ctx, A, B, pairs, ta, tb, *_ = Made.get()
    ssim = ctx.metrics_ragged(A, B, pairs, 3)[1].tolist()
    for i, (x, y) in enumerate(zip(ta, tb)):
        with np.errstate(invalid="ignore"):
            want = metrics.ssim(x, y).item()
        print(f"pair {i} {tuple(x.shape)}: {ssim[i]!r} / host {want!r} (diff {abs(ssim[i] - want):.3g})")
        if math.isnan(want):
            assert math.isnan(ssim[i]), i
        else:
            assert abs(ssim[i] - want) <= SSIM_BAR, (i, ssim[i], want)


def test_order_and_neighbours_do_not_matter():
    ctx, A, B, pairs, ta, tb, ref_sse, ref_ssim, _ = Made.get()
    perm = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(3)).tolist()
    assert perm != sorted(perm)
    sse, ssim = ctx.metrics_ragged(A, B, [pairs[i] for i in perm], 3)
    assert sse.tolist() == [ref_sse[i].item() for i in perm] and bits(ssim) == [bits(ref_ssim)[i] for i in perm]
    for i in (0, 6, 7, 9, CONST + 1):  # a pair alone
        sse, ssim = ctx.metrics_ragged(A, B, [pairs[i]], 3)
        assert sse.tolist() == [ref_sse[i].item()] and bits(ssim) == [bits(ref_ssim)[i]]


def test_squared_error_alone():
    ctx, A, B, pairs, ta, tb, ref_sse, *_ = Made.get()
    sse, ssim = ctx.metrics_ragged(A, B, pairs + [(3, 5, 1, 2)], 3, want_ssim=False)  # (without the SSIM a 3x5 pair is taken)
    assert ssim is None
    small = int(((A[1:46].long() - B[2:47].long()) ** 2).sum())
    assert sse.tolist() == ref_sse.tolist() + [small]


def test_results_hold_on_a_side_stream():
    ctx, A, B, pairs, ta, tb, ref_sse, ref_ssim, _ = Made.get()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sse, ssim = ctx.metrics_ragged(A, B, pairs, 3)
    s.synchronize()
    assert sse.tolist() == ref_sse.tolist() and bits(ssim) == bits(ref_ssim)
    sse, ssim = ctx.metrics_ragged(A, B, pairs, 3)  # and back on the default stream
    assert sse.tolist() == ref_sse.tolist() and bits(ssim) == bits(ref_ssim)


def test_the_list_form_uploads_and_scores():
    import lrf_amd
    ctx, A, B, pairs, ta, tb, ref_sse, ref_ssim, ref_psnr = Made.get()
    for la, lb in ((ta, tb), ([x.cuda() for x in ta], [y.cuda() for y in tb])):
        m = lrf_amd.image_metrics_ragged(la, lb)
        assert set(m) == {"sse", "mse", "psnr", "ssim"} and all(v.is_cuda and tuple(v.shape) == (len(ta),) for v in m.values())
        assert m["sse"].tolist() == ref_sse.tolist() and bits(m["ssim"]) == bits(ref_ssim) and bits(m["psnr"]) == bits(ref_psnr)
    m = lrf_amd.image_metrics_ragged(ta, tb, want_ssim=False)
    assert set(m) == {"sse", "mse", "psnr"} and m["sse"].tolist() == ref_sse.tolist()
    gray = lrf_amd.image_metrics_ragged([ta[4][:1], ta[8][1:2]], [tb[4][:1], tb[8][1:2]])  # C = 1
    want = [lrf_amd.image_metrics_batch(ta[i][c:c + 1][None], tb[i][c:c + 1][None]) for i, c in ((4, 0), (8, 1))]
    assert bits(gray["ssim"]) == bits(torch.cat([w["ssim"] for w in want])) and gray["sse"].tolist() == [w["sse"].item() for w in want]


def test_a_refused_call_leaves_its_outputs_untouched():
    from lrf_amd import _lib
    ctx, A, B, pairs, ta, tb, ref_sse, ref_ssim, _ = Made.get()
    lib = _lib.load()
    sse = torch.full((4,), 0x5A5A, dtype=torch.int64, device="cuda")
    ssim = torch.full((4,), 0.25, dtype=torch.float64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(n, ps, C=3, a_len=None, b_len=None, a=A, b=B, out=sse, want=ssim):
        arr = np.ascontiguousarray(np.array(ps, dtype=np.int64).reshape(-1, 4)) if ps is not None else None
        ctx.use_torch_stream()
        return lib.lrf_image_metrics_ragged_u8(ctx._h, n, ctypes.c_void_p(arr.ctypes.data) if arr is not None else None, C, ptr(a),
                                               A.numel() if a_len is None else a_len, ptr(b), B.numel() if b_len is None else b_len, ptr(out), ptr(want))
    ok = pairs[:3]
    H, W = ok[2][:2]
    einval = {
        "6 rows": call(3, ok[:2] + [(6, 30, 0, 0)]),
        "6 columns": call(3, ok[:2] + [(30, 6, 0, 0)]),
        "a range": call(3, ok[:2] + [(H, W, A.numel() - 3 * H * W + 1, 0)]),
        "b range": call(3, ok[:2] + [(H, W, 0, B.numel() - 3 * H * W + 1)]),
        "a_len short": call(3, ok, a_len=ok[2][2] + 3 * H * W - 1),
        "b_len short": call(3, ok, b_len=ok[2][3] + 3 * H * W - 1),
        "negative a": call(3, ok[:2] + [(H, W, -1, 0)]),
        "negative b": call(3, ok[:2] + [(H, W, 0, -1)]),
        "offset near 2^63": call(3, ok[:2] + [(H, W, 2 ** 63 - 1, 0)]),
        "n = 0": call(0, ok),
        "n = 65536": call(65536, ok),
        "C = 0": call(3, ok, C=0),
        "NULL pairs": call(3, None),
        "NULL a": call(3, ok, a=None),
        "NULL b": call(3, ok, b=None),
        "NULL sse": call(3, ok, out=None),
    }
    assert all(rc == -1 for rc in einval.values()), einval
    torch.cuda.synchronize()
    assert bool((sse == 0x5A5A).all()) and bool((ssim == 0.25).all()), "a refused call wrote to its output"
    assert call(3, ok) == 0
    assert sse[:3].tolist() == ref_sse[:3].tolist() and bits(ssim[:3]) == bits(ref_ssim[:3])
    assert sse[3].item() == 0x5A5A and ssim[3].item() == 0.25  # the call writes its n entries, no more
    for bad in ([(6, 30, 0, 0)], [(H, W, A.numel(), 0)], [], [(H, W, 0)]):
        with pytest.raises(ValueError):
            ctx.metrics_ragged(A, B, bad, 3)
    with pytest.raises(TypeError):
        ctx.metrics_ragged(A.float(), B, ok, 3)
