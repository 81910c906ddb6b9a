#!/usr/bin/env python3
"""Did a host-side change leave the device code alone?  Compares two device assembly files of the same translation unit, e.g.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S conv_f16.hip -o before.s     (parent commit)
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S conv_f16.hip -o after.s      (working tree)
    python tools/asm_kernel_diff.py before.s after.s

kernel by kernel, keyed by symbol: the instruction stream with its .amdhsa_* resource block, and the kernel's entry in the
code-object metadata (.vgpr_count, .sgpr_count, LDS, scratch, arguments).  The ORDER of the functions in the file follows the order
in which the host code instantiates the kernel templates, so a plain diff of the two files is not empty after a host refactor even
when every kernel is unchanged; the index of the function inside the module, which the compiler puts into local label names
(.LBB<index>_<block>), is normalised for the same reason, and comments are dropped (they repeat those labels).  Lines naming the
per-compile __hip_cuid_<hash> symbol and .file lines are ignored.  Exit status 0 = same symbols, same text per symbol."""
import re
import sys


def load(path):
    text = "".join(l for l in open(path) if "__hip_cuid_" not in l and not re.match(r"\s*\.file", l))
    head, _, meta = text.partition("\t.amdgpu_metadata")
    head, _, trailer = head.partition("\t.section\t.AMDGPU.gpr_maximums")
    parts = re.split(r"(?m)^(?=\s*\.section\s+\.text\.)", head)
    funcs = {}
    for chunk in parts[1:]:  # a function re-enters its own .text.<symbol> section after its kernel descriptor: join the pieces
        sym = re.match(r"\s*\.section\s+\.text\.([^,]+),", chunk).group(1)
        chunk = re.sub(r"\.(LBB|LJTI|LCPI|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1N", chunk)
        chunk = "\n".join(l for l in (x.split(";")[0].rstrip() for x in chunk.splitlines()) if l)
        funcs[sym] = funcs.get(sym, "") + chunk + "\n"
    entries = re.split(r"(?m)^(?=  - \.agpr_count)", meta)
    kernels = {re.search(r"\.name:\s+(\S+)", e).group(1): e.split("amdhsa.target:")[0] for e in entries[1:]}
    return {"preamble/trailer": {"": parts[0] + trailer}, "function": funcs, "metadata entry": kernels}


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    same = True
    for what in a:
        only = sorted(set(a[what]) ^ set(b[what]))
        differ = [k for k in a[what] if k in b[what] and a[what][k] != b[what][k]]
        if only:
            print(f"{what}: {len(only)} symbols on one side only, e.g. {only[:4]}")
        if differ:
            print(f"{what}: text differs for {len(differ)} symbols, e.g. {differ[:4]}")
        same = same and not only and not differ
    order = "same order" if list(a["function"]) == list(b["function"]) else "different order in the file"
    print(f"{len(a['function'])} functions, {len(a['metadata entry'])} kernels: {'identical per symbol' if same else 'DIFFERENT'} ({order})")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
