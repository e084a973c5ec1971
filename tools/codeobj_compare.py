"""Compares the gfx code objects inside two host objects (or libraries) built by hipcc, kernel by kernel: registers, spills, LDS,
scratch and kernel-argument bytes from the notes, and whether the machine code of each kernel that both have is byte-identical (sha1 of
the function's bytes in .text).  A Markdown table on stdout.

    python tools/codeobj_compare.py parent/vlr_fragpileup.hip.o varlociraptor_amd/csrc/build/default/vlr_fragpileup.hip.o
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_objects(path, tmp, tag):
    fat = os.path.join(tmp, tag + ".fat")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    d = open(fat, "rb").read()
    magic, out = b"__CLANG_OFFLOAD_BUNDLE__", []
    for st in [i for i in range(len(d)) if d.startswith(magic, i)]:
        n = struct.unpack_from("<Q", d, st + 24)[0]
        off = st + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", d, off)
            trip = d[off + 24: off + 24 + tl].decode()
            off += 24 + tl
            if "gfx" in trip and sz:
                p = os.path.join(tmp, "%s_%d.elf" % (tag, len(out)))
                open(p, "wb").write(d[st + o: st + o + sz])
                out.append(p)
    return out


def kernels(path, tmp, tag):
    """{demangled kernel name: (vgpr, sgpr, vspill, sspill, lds, scratch, kernarg, sha1 of its code)}"""
    out = {}
    for elf in code_objects(path, tmp, tag):
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", elf], capture_output=True, text=True).stdout
        meta = {}
        for blk in re.split(r"\n\s+- (?=\.a)", notes):
            nm = re.search(r"\.name:\s+(\S+)", blk)
            if not nm or ".vgpr_count" not in blk:
                continue
            g = lambda k: int((re.search(r"\.%s:\s+(\d+)" % k, blk) or [0, "0"])[1])
            meta[nm.group(1)] = (g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"),
                                 g("kernarg_segment_size"))
        text = subprocess.run([LLVM + "/llvm-readelf", "-SW", elf], capture_output=True, text=True).stdout
        m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", text)
        addr, off = int(m.group(1), 16), int(m.group(2), 16)
        data = open(elf, "rb").read()
        syms = subprocess.run([LLVM + "/llvm-readelf", "-sW", elf], capture_output=True, text=True).stdout
        for line in syms.split("\n"):
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[7] in meta:
                a, size = int(f[1], 16), int(f[2])
                code = data[off + a - addr: off + a - addr + size]
                name = subprocess.run(["c++filt", f[7]], capture_output=True, text=True).stdout.strip().split("(")[0]
                out[name] = meta[f[7]] + (hashlib.sha1(code).hexdigest()[:12], size)
    return out


def main():
    a_path, b_path = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(a_path, tmp, "a"), kernels(b_path, tmp, "b")
    print("| kernel | first: vgpr sgpr vspill sspill lds scratch kernarg, code bytes | second | machine code |")
    print("|---|---|---|---|")
    fmt = lambda v: "-" if v is None else "%d %d %d %d %d %d %d, %d" % (v[:7] + (v[8],))
    for name in sorted(set(a) | set(b)):
        x, y = a.get(name), b.get(name)
        same = "" if x is None or y is None else ("identical" if x[7] == y[7] and x[:7] == y[:7] else "DIFFERS")
        print("| `%s` | %s | %s | %s |" % (name, fmt(x), fmt(y), same))


if __name__ == "__main__":
    main()
