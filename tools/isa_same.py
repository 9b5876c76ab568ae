#!/usr/bin/env python3
"""Dev tool (no GPU needed): are the kernels of two builds of libfspann_hip.so the same machine code?

usage: python tools/isa_same.py PARENT.so NEW.so [-v]

Extracts the gfx950 code object of both libraries, disassembles them and compares, for EVERY kernel symbol the first library
has, the instruction stream (mnemonic + operands, in order; addresses and encodings are dropped, branch targets are relative
and therefore part of the operands).  A change that only adds instantiations (a new row type, say) must leave every existing
kernel instruction-for-instruction identical; kernels only the second library has are counted, not compared.
Prints one summary line; exit status 0 = all identical, 1 = some differ or are missing."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_isa(so):
    """{kernel symbol: [instruction, ...]} of the gfx950 code object inside `so`."""
    with tempfile.TemporaryDirectory() as td:
        lib = os.path.join(td, "lib.so")
        shutil.copy(so, lib)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", lib], check=True, capture_output=True, cwd=td)
        objs = [f for f in os.listdir(td) if "amdgcn" in f and "gfx950" in f]
        if len(objs) != 1:
            raise SystemExit(f"isa_same: {so}: expected one gfx950 code object, found {objs}")
        obj = os.path.join(td, objs[0])
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", obj], check=True, capture_output=True, text=True).stdout
        kernels = set(re.findall(r"\.name:\s+(\S+)", notes))
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--mcpu=gfx950", obj], check=True, capture_output=True,
                             text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:\s*$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in kernels else None
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        if ins and ins != "...":      # "...": objdump's elision of the zero padding behind a kernel (depends on what the linker placed next)
            cur.append(re.sub(r"\s+", " ", ins))
    return out


def main(argv):
    verbose = "-v" in argv
    args = [a for a in argv if a != "-v"]
    if len(args) != 2:
        raise SystemExit(__doc__)
    a, b = kernel_isa(args[0]), kernel_isa(args[1])
    same, differ, missing = [], [], []
    for name, ins in sorted(a.items()):
        if name not in b:
            missing.append(name)
        elif b[name] != ins:
            differ.append(name)
        else:
            same.append(name)
    if verbose or differ or missing:
        dem = dict(zip(differ + missing, subprocess.run(["c++filt"] + differ + missing, capture_output=True, text=True).stdout.splitlines()))
        for n in differ:
            x, y = a[n], b[n]
            at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            print(f"DIFFERS  {dem.get(n, n)}: {len(x)} vs {len(y)} instructions, first difference at #{at}: "
                  f"{x[at] if at < len(x) else '<end>'}  |  {y[at] if at < len(y) else '<end>'}")
        for n in missing:
            print(f"MISSING  {dem.get(n, n)}")
    ninstr = sum(len(a[n]) for n in same)
    print(f"isa_same: {len(a)} kernels in the first library: {len(same)} identical ({ninstr} instructions), {len(differ)} differ, "
          f"{len(missing)} missing; {len(set(b) - set(a))} kernels only in the second")
    return 0 if not differ and not missing else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
