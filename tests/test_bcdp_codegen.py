"""What the compiler made of k_bcd_p (no GPU needed): the gfx950 code objects of lrf_amd/liblrf_hip.so, disassembled.
  * no `flat_` memory instruction in any instantiation: only `global_` / `buffer_` sc1 loads may stand in for the acquire of
    the in-launch hand-offs (MI355X_MICROARCH.md, inter-workgroup visibility);
  * the rank <= 8 body (k_bcd_p<false, 0, *>) hands its partial slots, U spans and b tables over in 16-B sc1 stores, and
    its 4-byte sc1 stores are few: 59 / 38 in <false, 0, true> / <false, 0, false> before the dense slots and whole U
    spans; what is left is the V table (R words per row), the head / tail pieces of an unaligned U span and the queue's words."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lrf_amd", "liblrf_hip.so")
LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
MAX_DWORD_SC1_STORES = 20


def _code_objects(tmp_path):
    """The gfx950 code objects of every offload bundle in the library's .hip_fatbin section (one bundle per unit)."""
    fb = tmp_path / "fatbin.bin"
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", LIB, str(tmp_path / "stripped")])
    data = fb.read_bytes()
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl].decode()
            p += tl
            if triple.endswith("gfx950") and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 1)
    return out


@pytest.fixture(scope="module")
def bcdp_functions(tmp_path_factory):
    for tool in ("llvm-objcopy", "llvm-objdump"):
        assert os.path.exists(os.path.join(LLVM, tool)), f"{tool} of the ROCm toolchain is needed"
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build)"
    tmp = tmp_path_factory.mktemp("codegen")
    funcs = {}
    for i, co in enumerate(_code_objects(tmp)):
        path = tmp / f"co{i}.o"
        path.write_bytes(co)
        txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", str(path)], text=True)
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1) if m.group(1).startswith("_Z7k_bcd_p") else None
                if cur:
                    funcs[cur] = []
            elif cur and line.startswith("\t"):
                funcs[cur].append(line.strip().split("//")[0].strip())
    assert len(funcs) >= 12, sorted(funcs)  # <false,0,*>, <true,0,*>, <true,9..16,false>
    return funcs


def test_no_flat_memory_instructions(bcdp_functions):
    for name, ins in bcdp_functions.items():
        flat = [i for i in ins if i.startswith("flat_")]
        assert not flat, (name, flat[:5])


def test_rank8_body_stores_whole_chunks(bcdp_functions):
    low = {n: ins for n, ins in bcdp_functions.items() if n.startswith("_Z7k_bcd_pILb0ELi0E")}
    assert len(low) == 2, sorted(low)
    for name, ins in low.items():
        x4 = [i for i in ins if i.startswith("global_store_dwordx4 ") and "sc1" in i]
        assert len(x4) >= 3, (name, len(x4))  # partial slot, U span, b table
        dw = [i for i in ins if i.startswith("global_store_dword ") and "sc1" in i]
        assert len(dw) <= MAX_DWORD_SC1_STORES, (name, len(dw))
