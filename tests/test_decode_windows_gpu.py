"""GPU suite (-m gpu): what the ten C entries that decode crops say when they refuse a crop list.  The Python callers validate
first, so nothing else in the suite reaches these refusals: here each entry is called through ctypes with a table of bad lists,
and the return code, lrf_last_error — a literal string per row, the words the entries had before the checks moved into
check_windows (lrf_plan.cpp) and refuse_window (lrf_encode8.hip) — and the sentinel-filled output are asserted.  A refusal
launches nothing.  Two images, 24x48 and 45x61 at (7,3,3), and their gray twins at rank 7."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(24, 48), (45, 61)]
EINVAL = -1
# the good lists: three windows of 8x12 (the scaled shapes: at scale 2, where image 1 is 23x31), three boxes resized to 5x7
GOOD = {"crop": [(0, 0, 0), (1, 3, 5), (1, 14, 18)], "scaled": [(0, 2, 0, 0), (1, 2, 3, 5), (1, 2, 14, 18)],
        "resized": [(0, 0, 0, 24, 48, 0), (1, 37, 0, 8, 61, 1), (1, 3, 5, 11, 13, 0)]}
# body: (the entries' stem, gray, crop shape, the call's size, elements of the exact output)
BODIES = {"crops": ("lrf_qmf_decode_crops", False, "crop", (8, 12), 864), "scaled_crops": ("lrf_qmf_decode_scaled_crops", False, "scaled", (8, 12), 864),
          "resized_crops": ("lrf_qmf_decode_resized_crops", False, "resized", (5, 7), 315),
          "gray_crops": ("lrf_qmf_decode_gray_crops", True, "scaled", (8, 12), 288),
          "gray_resized_crops": ("lrf_qmf_decode_gray_resized_crops", True, "resized", (5, 7), 105)}
# row: (what differs from the good call — last: the crop that replaces crop 2; n_crops, size, short: elements missing —, the message)
ROWS = {
    "crops": [
        (dict(n_crops=0), "n_crops=0 out of range [1,2^20]"),
        (dict(n_crops=2 ** 20 + 1), "n_crops=1048577 out of range [1,2^20]"),
        (dict(size=(0, 12)), "crop size 0x12 out of range"),
        (dict(size=(8, 0)), "crop size 8x0 out of range"),
        (dict(size=(16385, 12)), "3 crops of 3x16385x12 leave the output buffer of 864 bytes"),
        (dict(last=(-1, 14, 18)), "crop 2: image -1 out of range [0,2)"),
        (dict(last=(2, 14, 18)), "crop 2: image 2 out of range [0,2)"),
        (dict(last=(1, -1, 18)), "crop 2: 8x12 at (-1,18) leaves image 1 of 45x61"),
        (dict(last=(1, 14, -1)), "crop 2: 8x12 at (14,-1) leaves image 1 of 45x61"),
        (dict(last=(1, 38, 18)), "crop 2: 8x12 at (38,18) leaves image 1 of 45x61"),
        (dict(last=(1, 14, 50)), "crop 2: 8x12 at (14,50) leaves image 1 of 45x61"),
        (dict(short=1), "3 crops of 3x8x12 leave the output buffer of 863 bytes"),
    ],
    "scaled_crops": [
        (dict(n_crops=0), "n_crops=0 out of range [1,2^20]"),
        (dict(n_crops=2 ** 20 + 1), "n_crops=1048577 out of range [1,2^20]"),
        (dict(size=(0, 12)), "crop size 0x12 out of range"),
        (dict(size=(8, 0)), "crop size 8x0 out of range"),
        (dict(size=(16385, 12)), "3 crops of 3x16385x12 leave the output buffer of 864 bytes"),
        (dict(last=(-1, 2, 14, 18)), "crop 2: image -1 out of range [0,2)"),
        (dict(last=(2, 2, 14, 18)), "crop 2: image 2 out of range [0,2)"),
        (dict(last=(1, 3, 14, 18)), "crop 2: scale 3: 2, 4 or 8 expected"),
        (dict(last=(1, 1, 14, 18)), "crop 2: scale 1: 2, 4 or 8 expected"),
        (dict(last=(1, 2, -1, 18)), "crop 2: 8x12 at (-1,18) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 14, -1)), "crop 2: 8x12 at (14,-1) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 16, 18)), "crop 2: 8x12 at (16,18) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 14, 20)), "crop 2: 8x12 at (14,20) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 8, 0, 0)), "crop 2: 8x12 at (0,0) leaves image 1 of 6x8 at scale 1/8"),
        (dict(short=1), "3 crops of 3x8x12 leave the output buffer of 863 bytes"),
    ],
    "resized_crops": [
        (dict(n_crops=0), "n_crops=0 out of range [1,2^20]"),
        (dict(n_crops=2 ** 20 + 1), "n_crops=1048577 out of range [1,2^20]"),
        (dict(size=(0, 7)), "output size 0x7 out of range [1,16384]"),
        (dict(size=(5, 0)), "output size 5x0 out of range [1,16384]"),
        (dict(size=(16385, 7)), "output size 16385x7 out of range [1,16384]"),
        (dict(size=(5, 16385)), "output size 5x16385 out of range [1,16384]"),
        (dict(last=(-1, 3, 5, 11, 13, 0)), "crop 2: image -1 out of range [0,2)"),
        (dict(last=(2, 3, 5, 11, 13, 0)), "crop 2: image 2 out of range [0,2)"),
        (dict(last=(1, 3, 5, 0, 13, 0)), "crop 2: box of 0x13: both sides must be >= 1"),
        (dict(last=(1, 3, 5, 11, 0, 0)), "crop 2: box of 11x0: both sides must be >= 1"),
        (dict(last=(1, -1, 5, 11, 13, 0)), "crop 2: 11x13 at (-1,5) leaves image 1 of 45x61"),
        (dict(last=(1, 3, -1, 11, 13, 0)), "crop 2: 11x13 at (3,-1) leaves image 1 of 45x61"),
        (dict(last=(1, 35, 5, 11, 13, 0)), "crop 2: 11x13 at (35,5) leaves image 1 of 45x61"),
        (dict(last=(1, 3, 49, 11, 13, 0)), "crop 2: 11x13 at (3,49) leaves image 1 of 45x61"),
        (dict(short=1), "3 crops of 3x5x7 leave the output buffer of 314 bytes"),
    ],
    "gray_crops": [
        (dict(n_crops=0), "n_crops=0 out of range [1,2^20]"),
        (dict(n_crops=2 ** 20 + 1), "n_crops=1048577 out of range [1,2^20]"),
        (dict(size=(0, 12)), "crop size 0x12 out of range"),
        (dict(size=(8, 0)), "crop size 8x0 out of range"),
        (dict(size=(16385, 12)), "3 crops of 16385x12 leave the output buffer of 288 elements"),
        (dict(last=(-1, 2, 14, 18)), "crop 2: image -1 out of range [0,2)"),
        (dict(last=(2, 2, 14, 18)), "crop 2: image 2 out of range [0,2)"),
        (dict(last=(1, 3, 14, 18)), "crop 2: scale 3: 1, 2, 4 or 8 expected"),
        (dict(last=(1, 2, -1, 18)), "crop 2: 8x12 at (-1,18) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 14, -1)), "crop 2: 8x12 at (14,-1) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 16, 18)), "crop 2: 8x12 at (16,18) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 2, 14, 20)), "crop 2: 8x12 at (14,20) leaves image 1 of 23x31 at scale 1/2"),
        (dict(last=(1, 1, 38, 18)), "crop 2: 8x12 at (38,18) leaves image 1 of 45x61 at scale 1/1"),
        (dict(short=1), "3 crops of 8x12 leave the output buffer of 287 elements"),
    ],
    "gray_resized_crops": [
        (dict(n_crops=0), "n_crops=0 out of range [1,2^20]"),
        (dict(n_crops=2 ** 20 + 1), "n_crops=1048577 out of range [1,2^20]"),
        (dict(size=(0, 7)), "output size 0x7 out of range [1,16384]"),
        (dict(size=(5, 0)), "output size 5x0 out of range [1,16384]"),
        (dict(size=(16385, 7)), "output size 16385x7 out of range [1,16384]"),
        (dict(size=(5, 16385)), "output size 5x16385 out of range [1,16384]"),
        (dict(last=(-1, 3, 5, 11, 13, 0)), "crop 2: image -1 out of range [0,2)"),
        (dict(last=(2, 3, 5, 11, 13, 0)), "crop 2: image 2 out of range [0,2)"),
        (dict(last=(1, 3, 5, 0, 13, 0)), "crop 2: box of 0x13: both sides must be >= 1"),
        (dict(last=(1, 3, 5, 11, 0, 0)), "crop 2: box of 11x0: both sides must be >= 1"),
        (dict(last=(1, -1, 5, 11, 13, 0)), "crop 2: 11x13 at (-1,5) leaves image 1 of 45x61"),
        (dict(last=(1, 3, -1, 11, 13, 0)), "crop 2: 11x13 at (3,-1) leaves image 1 of 45x61"),
        (dict(last=(1, 35, 5, 11, 13, 0)), "crop 2: 11x13 at (35,5) leaves image 1 of 45x61"),
        (dict(last=(1, 3, 49, 11, 13, 0)), "crop 2: 11x13 at (3,49) leaves image 1 of 45x61"),
        (dict(short=1), "3 crops of 5x7 leave the output buffer of 104 elements"),
    ],
}
BAD_FORMAT = "tensor format: dtype 7: LRF_T_F32, LRF_T_F16 or LRF_T_BF16 expected"


@pytest.fixture(scope="module")
def factors():
    """gray -> (the descriptor array, U, V): zero factors of the two images on the GPU"""
    from lrf_amd import _lib
    made = {}
    for gray in (False, True):
        desc, uo, vo = ((_lib.GrayImage if gray else _lib.RaggedImage) * 2)(), 0, 0
        for d, (H, W) in zip(desc, SIZES):
            d.H, d.W, d.u_off, d.v_off = H, W, uo, vo
            if gray:
                d.R = 7
                uo, vo = uo + 7 * _lib.chan_dims(H, W, 1, (8, 8))[2], vo + 7 * 64
            else:
                d.R[0], d.R[1], d.R[2] = 7, 3, 3
                uo, vo = uo + sum(p[4] * r for p, r in zip(_lib.plane_dims(H, W), (7, 3, 3))), vo + 13 * 64
        made[gray] = (desc, torch.zeros(uo, dtype=torch.int8, device="cuda"), torch.zeros(vo, dtype=torch.int8, device="cuda"))
    return made


@pytest.mark.parametrize("tensor", [False, True], ids=["u8", "tensor"])
@pytest.mark.parametrize("body", BODIES)
def test_the_entry_refuses_in_its_words_and_writes_nothing(factors, body, tensor):
    from lrf_amd import _lib
    ctx, lib = _lib.context(0), _lib.load()
    stem, gray, shape, good_size, fit = BODIES[body]
    desc, U, V = factors[gray]
    crop_type = {"crop": _lib.Crop, "scaled": _lib.ScaledCrop, "resized": _lib.ResizedCrop}[shape]
    es = 4 if tensor else 1  # (the tensor rows write float32)
    out = torch.full((fit * es,), 0xA5, dtype=torch.uint8, device="cuda")
    fmt = _lib.check_tensor_format(torch.float32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(last=None, n_crops=3, size=good_size, short=0, fmt=fmt):
        rows = GOOD[shape][:2] + [GOOD[shape][2] if last is None else last]
        crops = (crop_type * 3)()
        for c, row in zip(crops, rows):
            for (name, _), value in zip(crop_type._fields_, row):
                setattr(c, name, value)
        lead = (ctx._h, 2, desc, ptr(U), U.numel(), ptr(V), V.numel(), n_crops, crops, size[0], size[1])
        ctx.use_torch_stream()
        if tensor:
            return getattr(lib, stem + "_tensor")(*lead, ctypes.byref(fmt), ptr(out), (fit - short) * es)
        return getattr(lib, stem + ("_u8" if gray else "_rgb_u8"))(*lead, ptr(out), fit - short)

    rows = list(ROWS[body])
    if tensor:
        bad = _lib.check_tensor_format(torch.float32)
        bad.dtype = 7
        rows.append((dict(fmt=bad), BAD_FORMAT))
    for how, message in rows:
        rc = call(**how)
        said = lib.lrf_last_error().decode()
        print(f"{stem}{'_tensor' if tensor else ''} {how}: rc {rc}: {said}")
        assert rc == EINVAL and said == message, (how, rc, said)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # and the good list is taken: the table above refuses for the reasons it names
    assert call() == 0, lib.lrf_last_error().decode()
    torch.cuda.synchronize()
    assert not bool((out == 0xA5).all())
