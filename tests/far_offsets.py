"""Helpers of test_far_offsets_gpu.py: where the items of a descriptor table are placed in a buffer that passes 2^32 bytes, and
the sentinel pattern an output buffer carries between them.  Host-only arithmetic except `fill_pattern`, `gaps_untouched` and
`restore`, which work on a CUDA tensor in chunks."""
import numpy as np

P31, P32 = 2 ** 31, 2 ** 32
BIG = P32 + 2 ** 26  # bytes of a far buffer
PAT = 2 ** 24        # bytes of the sentinel block; BIG is a multiple of it
assert BIG % PAT == 0

# (H, W, ranks): one image per decode body and class of tests/test_decode_ragged_gpu.py — 32x272 and 64x96 the 16-aligned tile
# (classes 0 and 2), 40x272 and 24x48 the strip body (classes 1, 3, 4), 45x61 at ranks <= 8 the r8 body, 173x264 and a rank
# above 32 the any-size body
EIGHT = [(32, 272, (7, 3, 3)), (40, 272, (8, 8, 5)), (45, 61, (7, 3, 3)), (64, 96, (12, 6, 6)), (24, 48, (16, 9, 16)), (173, 264, (5, 17, 2)),
         (40, 272, (32, 16, 16)), (24, 48, (33, 4, 4))]


def roles(s, variant):
    """the eight places an item of s bytes can take in a buffer of BIG bytes.  Variant 0: starts at 0; in the middle of the
    first half; ends at byte P31 - 1; starts exactly at P31; between P31 and P32; a MiB below P32; straddles P32 by two
    bytes (ends at P32 + 1); starts at P32 + 3.  Variant 1 (what variant 0 cannot hold without overlap): starts at 8; straddles
    P31 at its middle; a MiB above P31; straddles P32 a third in; 16 MiB above P32; odd places at 2^30 + 1 and 3 * 2^30 - 3; ends
    with the buffer.  Places that are multiples of 8 keep the 16-aligned decode body, the others move the image to another."""
    assert 0 < s <= 2 ** 19
    if variant == 0:
        return [0, P31 // 2 + 16, P31 - s, P31, P31 + P31 // 2 + 8, P32 - 2 ** 20, P32 + 2 - s, P32 + 3]
    return [8, P31 - s // 2 // 8 * 8, P31 + 2 ** 20, P32 - s // 3, P32 + 2 ** 24, 2 ** 30 + 1, 3 * 2 ** 30 - 3, BIG - s]


def place(sizes, variant, rot):
    """item i of `sizes` (bytes) at role (i + rot) % 8 of the variant -> int64 offsets, no two items sharing a byte"""
    assert len(sizes) == 8
    offs = np.array([roles(int(s), variant)[(i + rot) % 8] for i, s in enumerate(sizes)], dtype=np.int64)
    order = np.argsort(offs)
    ends = offs + np.asarray(sizes, dtype=np.int64)
    assert offs.min() >= 0 and ends.max() <= BIG
    assert all(ends[a] <= offs[b] for a, b in zip(order, order[1:])), "two items overlap"
    return offs


def covers(offs, sizes):
    """does the placement straddle or start at P31, straddle P32 and start past it?  (Variant 0's starts at 0, at P32 + 3 and its
    end at P31 - 1 are `roles`' by construction.)"""
    o, e = np.asarray(offs, dtype=np.int64), np.asarray(offs, dtype=np.int64) + np.asarray(sizes, dtype=np.int64)
    return bool(((o < P32) & (e > P32)).any() and (o > P32).any() and ((o == P31) | ((o < P31) & (e > P31))).any())


def compact(offs, sizes, align=16):
    """the same items back to back in a small buffer, each keeping its place's residue modulo `align` (so the same decode body
    serves it) -> (offsets, bytes of the buffer)"""
    out, at = [], 0
    for o, s in zip(offs, sizes):
        at = (at + align - 1) // align * align + int(o) % align
        out.append(at)
        at += int(s)
    return np.array(out, dtype=np.int64), at + align


def fill_pattern(out, pat):
    """out (uint8, BIG bytes on the device) := pat repeated"""
    assert out.numel() == BIG and pat.numel() == PAT
    out.view(BIG // PAT, PAT).copy_(pat[None].expand(BIG // PAT, PAT))


def _touched_chunks(ranges):
    return sorted({k for a, b in ranges for k in range(int(a) // PAT, (int(b) - 1) // PAT + 1)})


def gaps_untouched(out, pat, ranges):
    """does every byte of `out` outside the (start, end) ranges still carry the pattern?  Compared on the device chunk by chunk"""
    import torch
    rows = out.view(BIG // PAT, PAT)
    hit = set(_touched_chunks(ranges))
    bad = torch.zeros((), dtype=torch.bool, device=out.device)
    clean = [k for k in range(BIG // PAT) if k not in hit]
    for k0 in range(0, len(clean), 16):
        idx = clean[k0:k0 + 16]
        if idx[-1] - idx[0] == len(idx) - 1:
            bad |= (rows[idx[0]:idx[-1] + 1] != pat).any()
        else:
            for k in idx:
                bad |= (rows[k] != pat).any()
    for k in hit:
        diff = rows[k] != pat
        for a, b in ranges:
            lo, hi = max(int(a), k * PAT), min(int(b), (k + 1) * PAT)
            if lo < hi:
                diff[lo - k * PAT:hi - k * PAT] = False
        bad |= diff.any()
    return not bool(bad)


def restore(out, pat, ranges):
    """puts the pattern back where a call wrote"""
    rows = out.view(BIG // PAT, PAT)
    for k in _touched_chunks(ranges):
        rows[k].copy_(pat)
