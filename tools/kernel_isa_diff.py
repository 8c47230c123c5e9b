"""Which kernels of two builds of one source file compile to different instructions (no GPU needed).

usage: python tools/kernel_isa_diff.py <old.o> <new.o>     (hipcc host objects, e.g. csrc/build_base/conv.o csrc/build/conv.o)

Extracts the gfx950 code object of each host object, disassembles it and compares the instruction text kernel by
kernel.  Two kinds of difference do not count as a change of code: PC-relative offsets to globals
(`s_add_u32 sN, sN, <literal>` after `s_getpc`) and the offsets of `s_load_dword*` from the kernarg pointer
(hidden arguments move when an argument struct grows).  A kernel whose template argument list only gained
defaulted arguments (`<5>` -> `<5, 0>`) is matched with its old self.  Used to check that the kernels a change
must leave alone kept their instructions (the GDN epilogue fusion).
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def disasm(obj):
    with tempfile.TemporaryDirectory() as t:
        fb, co = os.path.join(t, "fb"), os.path.join(t, "co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(t, "x.o")],
                       check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
                        f"--targets={TARGET}", f"--output={co}"], check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                              capture_output=True, text=True).stdout
    names = subprocess.run(["c++filt"], input=text, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in names.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", re.sub(r"//.*", "", line)).strip()
            ins = re.sub(r"<[^>]*>", "", ins)                                  # branch-target symbols
            ins = re.sub(r"^(s_add_u32 s\d+, s\d+), 0x[0-9a-f]+$", r"\1, PCREL", ins)
            ins = re.sub(r"^(s_load_dword\w* \S+ s\[\d+:\d+\]), 0x[0-9a-f]+$", r"\1, KERNARG", ins)
            cur.append(re.sub(r"\s+", " ", ins))
    return kernels


def base_name(k):
    """`name<5, 0>(args)` -> `name`: the key that survives defaulted template arguments."""
    return re.sub(r"<.*", "", k)


def main():
    old, new = disasm(sys.argv[1]), disasm(sys.argv[2])
    same = diff = 0
    for k, body in sorted(old.items()):
        cand = [k] if k in new else [n for n in new if base_name(n) == base_name(k) and len(new[n]) == len(body)
                                     and n not in old]
        hit = next((n for n in cand if new[n] == body), None)
        if hit is not None:
            same += 1
            if hit != k:
                print(f"SAME (renamed) {k}  ->  {hit}")
        else:
            diff += 1
            print(f"DIFF {k}" if cand else f"GONE {k}")
    added = [n for n in new if n not in old]
    print(f"{same} of {len(old)} kernels keep their instructions, {diff} differ or are gone, {len(added)} new names")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
