"""CPU suite of the inflate of factor columns: the host restatement lrf_pack_inflate_column_i8 (lrf_amd/csrc/lrf_inflate_shared.h,
the routine the kernel runs per lane) against zlib.decompress on the corpus, the hand-built streams and CORRUPT; the column
index lrf_pack_index_qmf_columns_ragged; and the stand-alone sanitizer program over the same streams."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as dc
import inflate_cases as ic
from conftest import ROOT


def test_kernel_id_of_the_binding_is_the_header_one():
    """LRF_K_INFLATE is spelled as LRF_K_COUNT in the header (the ids below LRF_K_COUNT are pinned by older tests), so the guard
    that keeps the Python constants in step with the header does not see it: this one does"""
    import re
    from lrf_amd import _lib
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    count = int(re.search(r"#define\s+LRF_K_COUNT\s+(\d+)", header).group(1))
    assert re.search(r"#define\s+LRF_K_INFLATE\s+LRF_K_COUNT\b", header)
    slots = re.search(r"#define\s+LRF_K_SLOTS\s+\(LRF_K_COUNT \+ (\d+)\)", header)
    assert slots and _lib.LRF_K_INFLATE == count < count + int(slots.group(1))
    assert _lib.LRF_K_INFLATE not in _lib.KERNEL_NAMES  # (the names bench.py prints are those of the ids below LRF_K_COUNT)


def test_every_refusal_rule_has_its_stream_and_its_status():
    header = open(os.path.join(ROOT, "include", "lrf_hip.h")).read()
    import re
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+LRFI_E_([A-Z]+)\s+(\d+)", header)}
    assert len(set(codes.values())) == len(codes) and min(codes.values()) > 0
    got = {ic.host_inflate(z, rows)[0] for _, z, rows in ic.refusals()}
    assert got == set(codes.values()) - {codes["CAP"]}  # (the cap cannot be reached: every step consumes or produces)


@pytest.mark.parametrize("stride", [1, 3, 33])
def test_corpus_and_hand_built_streams_inflate_to_zlibs_bytes(stride):
    for name, z, data in ic.corpus() + ic.hand_built():
        rc, col = ic.host_inflate(z, len(data), stride)
        assert rc == 0 and col.tobytes() == data, (name, rc)


def check_against_zlib(name, z, rows, stride=1):
    want = ic.zlib_verdict(z, rows)
    rc, col = ic.host_inflate(z, rows, stride)  # (asserts guards and padding whatever the status)
    assert (rc != 0) == (want is None), (name, rc)
    if want is not None:
        assert col.tobytes() == want, name


def test_corrupt_streams_are_refused_exactly_when_zlib_refuses_them():
    for name, z, rows in ic.corrupt():
        for stride in (1, 3):
            check_against_zlib(name, z, rows, stride)


def test_rows_off_by_one_in_both_directions():
    for name, z, data in ic.corpus() + ic.hand_built():
        for rows in (len(data) - 1, len(data) + 1):
            if rows >= 1:
                rc, _ = ic.host_inflate(z, rows, 2)
                assert rc != 0, (name, rows)


def test_bad_arguments():
    lib = ic.pack_lib()
    buf = np.zeros(8, dtype=np.int8)
    z = ic.hand_built()[0][1]
    assert lib.lrf_pack_inflate_column_i8(z, len(z), buf.ctypes.data, 0, 1) == -1
    assert lib.lrf_pack_inflate_column_i8(z, len(z), buf.ctypes.data, 8, 0) == -1
    assert lib.lrf_pack_inflate_column_i8(z, -1, buf.ctypes.data, 8, 1) == -1
    assert lib.lrf_pack_inflate_column_i8(None, 4, buf.ctypes.data, 8, 1) == -1
    assert lib.lrf_pack_inflate_column_i8(z, len(z), None, 8, 1) == -1


# ---- the column index -------------------------------------------------------------------------------------------------------
def index(blobs, Ms, Rs, ncols=None):
    n = len(blobs)
    total = 2 * sum(r for R in Rs for r in R)
    ncols = total if ncols is None else ncols
    off, ln = np.full(max(total, 1), -7, dtype=np.int64), np.full(max(total, 1), -7, dtype=np.int32)
    rc = ic.pack_lib().lrf_pack_index_qmf_columns_ragged(
        (ctypes.c_char_p * n)(*blobs), (ctypes.c_int64 * n)(*[len(b) for b in blobs]), n,
        (ctypes.c_int64 * (3 * n))(*[m for M in Ms for m in M]), (ctypes.c_int * (3 * n))(*[r for R in Rs for r in R]), off.ctypes.data, ln.ctypes.data, ncols)
    return rc, off, ln


def default_branch_streams():
    """[(stream, M, R)]: the golden fixtures' own streams of the default branch, and the same factors in the containers
    deflate="device" encoders write"""
    from lrf_amd import _lib
    from lrf_amd.container import bytes_to_dict, separate_bytes
    out = []
    golden = {name: fac for name, fac in dc.golden_factor_sets()}
    for name, fac in golden.items():
        enc = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["encoded"].tobytes()
        head = separate_bytes(enc, 2)[0]
        meta = bytes_to_dict(head)
        if meta.get("color space") != "YCbCr" or not meta.get("patch") or list(meta.get("patch size", [])) != [8, 8]:
            continue
        H, W = meta["original size"][0]
        M = [d[4] for d in _lib.plane_dims(int(H), int(W))]
        R = [int(r) for r in meta["rank"]]
        if [f.shape for f in fac] != [s for m, r in zip(M, R) for s in ((m, r), (64, r))]:
            continue
        out.append((enc, M, R))
        if len(out) <= 6:
            out.append((ic.deflated_container(fac, bytes(head)), M, R))
    assert len(out) >= 6
    return out


def test_index_reproduces_the_boundaries_separate_bytes_gives():
    from lrf_amd.container import separate_bytes
    cases = default_branch_streams()
    blobs = [bytes(separate_bytes(s, 2)[1]) for s, _, _ in cases]
    rc, off, ln = index(blobs, [M for _, M, _ in cases], [R for _, _, R in cases])  # all of them in one ragged call
    assert rc == 0
    k = 0
    for blob, (_, M, R) in zip(blobs, cases):
        last_end = 0
        for f, mat in enumerate(separate_bytes(blob, 6)):
            for fiber in separate_bytes(separate_bytes(mat, 2)[1], R[f // 2]):
                assert blob[off[k]:off[k] + ln[k]] == bytes(fiber) and off[k] >= last_end
                rows = 64 if f % 2 else M[f // 2]
                assert ic.host_inflate(blob[off[k]:off[k] + ln[k]], rows)[0] == 0
                last_end = off[k] + ln[k]
                k += 1
    assert k == off.size


def test_index_refuses_what_the_unpacker_refuses():
    from lrf_amd.container import combine_bytes, separate_bytes
    s, M, R = default_branch_streams()[0]
    blob = bytes(separate_bytes(s, 2)[1])
    assert index([blob], [M], [R])[0] == 0
    assert index([blob[:len(blob) // 2]], [M], [R])[0] == -6 and index([blob[:3]], [M], [R])[0] == -6 and index([b""], [M], [R])[0] == -6
    # (the fold gives its last payload no length: a blob that lost its last byte still walks, and the last column's stream is short)
    rc, off, ln = index([blob[:-1]], [M], [R])
    assert rc == 0 and ic.host_inflate(blob[off[-1]:off[-1] + ln[-1]], 64)[0] != 0
    assert index([blob], [M], [[R[0] + 1, R[1], R[2]]])[0] == -6  # num_fibers is not the rank
    mats = [bytes(m) for m in separate_bytes(blob, 6)]
    for old, new in ((b'"dtype": "int8"', b'"dtype": "int16"'), (b'"mode": "col"', b'"mode": "row"')):
        head, body = separate_bytes(mats[2], 2)
        assert old in bytes(head)
        bad = mats[:2] + [bytes(combine_bytes([bytes(head).replace(old, new), bytes(body)]))] + mats[3:]
        assert index([bytes(combine_bytes(bad))], [M], [R])[0] == -6
    assert index([blob], [M], [R], ncols=2 * sum(R) + 1)[0] == -1


# ---- the sanitizer program --------------------------------------------------------------------------------------------------
def test_sanitizer_program_is_clean_over_every_stream(tmp_path):
    """tools/inflate_san_main.cpp: the shared routine and lrf_pack.cpp's entry under ASan and UBSan, as a program of its own"""
    exe, data = str(tmp_path / "inflate_san"), str(tmp_path / "streams.bin")
    # (the sanitizer runtimes linked statically: the program needs nothing from the environment it is started in)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tools", "inflate_san_main.cpp"), "-lz"])
    n = ic.dump(data)
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{n} streams" in r.stdout
