#!/usr/bin/env python3
"""Registers, scratch (spills) and LDS of every kernel in built objects (default build/obj/*.o), from the code objects' metadata
notes: `python tools/kernel_resources.py [objects] > file` -- diff two builds to see what a change cost a kernel's register budget.
`--disasm DIR` also writes every kernel's disassembly to DIR/<demangled name>.s with the kernel's own symbol (and the address
column of branch comments) replaced by a placeholder: `diff -r` of two builds' directories shows which kernels a change moved."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
TARGET = "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"


def device_code_object(path: str, td: str):
    """the gfx950 code object bundled in a host object / shared library, or None"""
    co = os.path.join(td, "dev.co")
    fat = os.path.join(td, "fat.bin")
    r = subprocess.run([LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat], capture_output=True)
    if r.returncode != 0 or not os.path.isfile(fat) or os.path.getsize(fat) == 0:
        return None
    r = subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", TARGET, f"--output={co}"],
                       capture_output=True)
    return co if r.returncode == 0 and os.path.isfile(co) and os.path.getsize(co) else None


def dump_disasm(co: str, outdir: str):
    """one file per kernel: the llvm-objdump text between the kernel's label and the next symbol's"""
    txt = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    parts = re.split(r"^<([^>\n]+)>:\n", txt, flags=re.M)          # [head, sym, body, sym, body, ...]
    syms = parts[1::2]
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    os.makedirs(outdir, exist_ok=True)
    for sym, name, body in zip(syms, names, parts[2::2]):
        body = re.sub(r"// [0-9A-F]+: [0-9A-F ]+", "// ", body.replace(sym, "KERNEL"))
        body = re.sub(r"(\s*\.\.\.\s*)+$", "\n", body)                      # (padding up to the next symbol)
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        with open(os.path.join(outdir, name + ".s"), "w") as f:
            f.write(body)


def main():
    args = sys.argv[1:]
    disasm = None
    if "--disasm" in args:
        i = args.index("--disasm")
        disasm = args[i + 1]
        del args[i:i + 2]
    paths = args or sorted(glob.glob("build/obj/*.o"))       # one code object per translation unit
    rows = []
    for path in paths:
        with tempfile.TemporaryDirectory() as td:
            co = device_code_object(path, td)
            if co is None:
                continue
            if disasm:
                dump_disasm(co, disasm)
            txt = subprocess.run([LLVM + "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in txt.split("- .agpr_count:")[1:]:
            def g(k):
                m = re.search(rf"\.{k}:\s*(\S+)", blk)
                return m.group(1) if m else "?"
            rows.append((g("name"), g("vgpr_count"), blk.split("\n")[0].strip(), g("sgpr_count"), g("private_segment_fixed_size"),
                         g("group_segment_fixed_size"), g("vgpr_spill_count")))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        print(f"{n[:160]:160s} vgpr {r[1]:>4s} agpr {r[2]:>4s} sgpr {r[3]:>4s} scratch {r[4]:>5s} lds {r[5]:>6s} spills {r[6]:>4s}")


if __name__ == "__main__":
    main()
