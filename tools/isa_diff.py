#!/usr/bin/env python3
"""isa_diff.py [-v] [--rename OLD=NEW ...] <tree A> <tree B> [name.hip ...] -- are the gfx950 kernels of two trees the same code?

Compiles every mvs_gi_amd/csrc/*.hip of both trees (or only the named ones) to device assembly with the flags of
__graft_entry__, drops what differs between any two compiles (the __hip_cuid_<hash> symbol, .ident, .file) and the
function ordinal in local labels (a kernel's position in its unit, which changes when a neighbour is added or removed), and compares
the text kernel by kernel: instructions, labels and the .amdhsa_* resource block.  --rename substitutes OLD by NEW in tree
A's assembly first (a kernel whose mangled name changed, e.g. a template list that got shorter, then compares as the same
kernel).  Needs no GPU.  Exit status 0 only when every kernel is identical and none was added or removed."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import EXTRA_FLAGS  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# what __graft_entry__._compile_objects passes (written inline there), device side only, to assembly instead of an object
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only", "-S"]
OTHER = "(outside kernels)"


def assemble(job):
    root, name, out, renames = job
    src = os.path.join(root, "mvs_gi_amd", "csrc", name)
    r = subprocess.run([HIPCC] + FLAGS + EXTRA_FLAGS.get(name, []) + [src, "-o", out], stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit(f"{src}:\n{r.stderr}")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(out).read())
    # local labels carry the function's ordinal within the unit (.LBB<n>_<block>, .Lfunc_end<n>): a kernel added, removed or moved in
    # front of another renumbers it without changing its code
    text = re.sub(r"(\.LBB|\bBB)\d+_(\d+)", r"\1_\2", re.sub(r"\bLfunc_(begin|end)\d+", r"Lfunc_\1", text))
    for old, new in renames:
        text = text.replace(old, new)
    return [ln for ln in text.splitlines() if not ln.lstrip().startswith((".ident", ".file"))]


def kernels(lines):
    """{kernel symbol: its lines, from the directives in front of its .type line (.section, .globl, .p2align: they name this
    kernel, not the one before it) to the next kernel's}; what precedes the first kernel and the metadata note behind the last
    one go under OTHER."""
    names = {ln.split()[1] for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")}
    out, cur = {OTHER: []}, OTHER
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m and m.group(1) in names:
            head = []
            while out[cur] and out[cur][-1].lstrip().startswith((".section", ".globl", ".weak", ".protected", ".hidden", ".p2align")):
                head.insert(0, out[cur].pop())
            cur = m.group(1)
            out[cur] = head
        elif ln.lstrip().startswith(".amdgpu_metadata") or re.match(r"\s*\.type\s+\S+,@object", ln):
            cur = OTHER
        out[cur].append(ln)
    return out


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    verbose = "-v" in argv
    renames = [tuple(argv[i + 1].split("=", 1)) for i, x in enumerate(argv) if x == "--rename"]
    argv = [x for i, x in enumerate(argv) if x not in ("-v", "--rename") and (i == 0 or argv[i - 1] != "--rename")]
    a, b, only = os.path.abspath(argv[0]), os.path.abspath(argv[1]), set(argv[2:])
    files = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(r, "mvs_gi_amd", "csrc", "*.hip"))
                    if not only or os.path.basename(p) in only) for r in (a, b)]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        jobs = [(r, n, os.path.join(tmp, f"{i}_{n}.s"), [] if i else renames) for i, r in enumerate((a, b)) for n in files[i]]
        asm = dict(zip([(j[0], j[1]) for j in jobs], ex.map(assemble, jobs)))
    count, rest = {"identical": 0, "differs": 0, "added": 0, "removed": 0}, 0
    for n in sorted(set(files[0]) | set(files[1])):
        ka, kb = (kernels(asm.get((r, n), [])) for r in (a, b))
        if ka.pop(OTHER) != kb.pop(OTHER) and n in files[0] and n in files[1]:
            rest += 1
            print(f"differs   {n}: text outside the kernels")
        for k in sorted(set(ka) | set(kb)):
            state = "removed" if k not in kb else "added" if k not in ka else "identical" if ka[k] == kb[k] else "differs"
            count[state] += 1
            if state != "identical" or verbose:
                print(f"{state:9s} {n}: {k}" + (f" ({len(ka[k])} -> {len(kb[k])} lines)" if state == "differs" else ""))
    total = sum(count.values())
    print(f"isa_diff: {len(set(files[0]) | set(files[1]))} translation units, {total} kernels: " +
          ", ".join(f"{v} {k}" for k, v in count.items()) + f"; text outside the kernels differs in {rest} units")
    return 0 if count["identical"] == total and not rest else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
