"""Compare the gfx950 device code of two builds of liblrf_hip.so: `python tools/dev_codegen_diff.py A.so B.so [out.json]`.
Per code object of the .hip_fatbin section (extracted like tests/test_bcdp_codegen.py does): the set of kernel symbols, a hash of
every function's disassembly (addresses and comments stripped) and each kernel's resource notes (VGPRs, SGPRs, LDS, scratch)
from llvm-readelf --notes.  Prints "identical" or the differing names; the JSON holds the per-kernel list of both builds.
A host-side refactor must leave all of it equal."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def code_objects(lib, tmp):
    fb = os.path.join(tmp, "fatbin.bin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", lib, os.path.join(tmp, "stripped")])
    data = open(fb, "rb").read()
    out, pos = [], data.find(MAGIC)
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


def describe(lib):
    """{function or kernel name: {"code": sha1 of its instructions, note keys...}} over all code objects (names are unique per library)"""
    funcs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib, tmp)):
            path = os.path.join(tmp, f"co{i}.o")
            open(path, "wb").write(co)
            cur = None
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", path], text=True).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = funcs.setdefault(f"{m.group(1)}", {"object": i, "h": hashlib.sha1()})
                elif cur is not None and line.startswith("\t"):
                    cur["h"].update(line.strip().split("//")[0].strip().encode() + b"\n")
            name = None
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", path], text=True).splitlines():
                m = re.match(r"^\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", line)
                if not m:
                    continue
                if m.group(1) == ".name":
                    name = m.group(2)
                elif m.group(1) == ".symbol":
                    name = m.group(2)[:-3] if m.group(2).endswith(".kd") else m.group(2)
                elif m.group(1) in NOTE_KEYS and name in funcs:
                    funcs[name][m.group(1)] = int(m.group(2))
    return {k: dict({kk: vv for kk, vv in v.items() if kk != "h"}, code=v["h"].hexdigest()) for k, v in funcs.items()}


if __name__ == "__main__":
    a, b = describe(sys.argv[1]), describe(sys.argv[2])
    diff = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    kernels = sum(1 for v in a.values() if ".vgpr_count" in v)
    verdict = "identical" if not diff else "differ: " + ", ".join(diff)
    print(f"{len(a)} functions ({kernels} kernels with resource notes) in {1 + max(v['object'] for v in a.values())} code objects: {verdict}")
    if len(sys.argv) > 3:
        json.dump({"a": sys.argv[1], "b": sys.argv[2], "verdict": verdict, "functions_a": a, "functions_b": b}, open(sys.argv[3], "w"), indent=0, sort_keys=True)
    sys.exit(1 if diff else 0)
