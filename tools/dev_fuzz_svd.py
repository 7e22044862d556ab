"""Fuzz of svd_encode (RGB branch, 8x8 patches, uint8 factors: the byte-matrix path for ranks <= 8, the fp32-matrix path above)
against the oracle run the way the library runs, byte for byte (development aid; the logic of
tests/test_svd_any.py::test_svd_encode_equals_oracle_bytes).  Now and then a case is a batch of 2 or 3 images through
Context.svd_encode_rgb, or an image with more than 1536 patch rows (more than one chunk of k_gram192_u8, a partial last one).
python tools/dev_fuzz_svd.py [cases] [seed]"""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np, torch, lrf_amd
from lrf_amd import _lib
from lrf_amd.container import combine_bytes, dict_to_bytes, encode_tensor
from oracle import oracle
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
# batches and long matrices come from a stream of their own: the single-image cases of a seed stay what they were
rng2 = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 1, 1])
bad = 0


def image(kind, H, W, g):
    if kind == 0:
        return torch.from_numpy(g.integers(0, 256, (3, H, W), dtype=np.uint8))
    if kind == 1:
        base = torch.from_numpy(g.random((1, 3, max(H // 8, 1), max(W // 8, 1))).astype(np.float32)) * 255
        return (torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)[0]
                + torch.from_numpy(g.normal(0, 3, (3, H, W)).astype(np.float32))).clamp(0, 255).to(torch.uint8)
    return torch.full((3, H, W), int(g.integers(0, 256)), dtype=torch.uint8)


def expected(img, rank):
    X = oracle.rgb_matrix_any(img.numpy(), (8, 8))
    u, v = oracle.svd_topr_u8(X, rank)
    return X.shape[0], oracle.quantize_u8(u), oracle.quantize_u8(v)


for case in range(cases):
    H, W = int(rng.integers(8, 260)), int(rng.integers(8, 330))
    kind = int(rng.integers(0, 3))
    img = image(kind, H, W, rng)
    rank = int(rng.integers(1, 14))
    enc = lrf_amd.svd_encode(img, rank=rank)
    M, (qu, su, mu), (qv, sv, mv) = expected(img, rank)
    Hp, Wp = H + (8 - H % 8) % 8, W + (8 - W % 8) % 8
    metadata = {"dtype": "uint8", "color space": "RGB", "patch": True, "patch size": (8, 8), "original size": [H, W], "padded size": [Hp, Wp]}
    metadata["quantization"] = {"u": [su, mu], "v": [sv, mv]}
    want = combine_bytes([dict_to_bytes(metadata), combine_bytes([encode_tensor(np.ascontiguousarray(f)) for f in (qu, qv)])])
    if enc != want:
        bad += 1
        print(f"MISMATCH case {case}: {H}x{W} rank {rank} kind {kind} (M={M})", flush=True)
    if case % 4 == 3:  # every fourth case: a batch of 1..3 images in one call, every other one of them past one chunk of rows
        B = int(rng2.integers(1, 4))
        if case % 8 == 7:
            H2 = int(rng2.integers(8, 41))  # more than 1536 patch rows: 2 .. 4 chunks, the last one partial
            W2 = 8 * (1536 // ((H2 + 7) // 8) + int(rng2.integers(1, 600))) + int(rng2.integers(0, 8))
        else:
            H2, W2 = int(rng2.integers(4, 80)), int(rng2.integers(4, 80))
        imgs = torch.stack([image(int(rng2.integers(0, 3)), H2, W2, rng2) for _ in range(B)])
        rank2 = int(rng2.integers(1, 14))
        ctx = _lib.context(None)
        U, V, qp = ctx.svd_encode_rgb(imgs.cuda(ctx.device), rank2)
        U, V, qp = U.cpu().numpy(), V.cpu().numpy(), qp.cpu().numpy()
        for b in range(B):
            M2, (qu, su, mu), (qv, sv, mv) = expected(imgs[b], rank2)
            if not (np.array_equal(U[b], qu) and np.array_equal(V[b], qv)
                    and np.array_equal(qp[b].view(np.int32), np.array([su, mu, sv, mv], np.float32).view(np.int32))):
                bad += 1
                print(f"MISMATCH case {case}: batch of {B}, image {b}: {H2}x{W2} rank {rank2} (M={M2})", flush=True)
print(f"done: {cases} cases, {bad} mismatches")
sys.exit(1 if bad else 0)
