#!/usr/bin/env python3
"""Dev tool (no GPU needed): are the kernels of two builds of libfspann_hip.so the same machine code?

usage: python tools/isa_same.py PARENT.so NEW.so [-v] [--map FILE]

Extracts the gfx950 code object of both libraries, disassembles them and compares, for EVERY kernel symbol the first library
has, the instruction stream (mnemonic + operands, in order; addresses and encodings are dropped, branch targets are relative
and therefore part of the operands).  A change that only adds instantiations (a new row type, say) must leave every existing
kernel instruction-for-instruction identical; kernels only the second library has are counted, not compared.

--map FILE: kernels that were renamed.  Each line is OLD<TAB>NEW; each side is a fragment matched as `fspann::FRAGMENT(` in the
demangled name and must hit exactly one kernel of its library.  The first library's kernel is then compared with that one.

A kernel that is not identical is EQUIVALENT when it has the same number of instructions, the same multiset of mnemonics and the
same vgpr_count, sgpr_count, group_segment_fixed_size and private_segment_fixed_size in the code object's notes (operands
commuted, independent neighbours swapped): it is reported by name with its differing lines and does not fail the run.
Prints one summary line; exit status 0 = all identical or equivalent, 1 = some differ or are missing."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernel_isa(so):
    """({kernel symbol: [instruction, ...]}, {kernel symbol: {META field: value}}) of the gfx950 code object inside `so`."""
    with tempfile.TemporaryDirectory() as td:
        lib = os.path.join(td, "lib.so")
        shutil.copy(so, lib)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", lib], check=True, capture_output=True, cwd=td)
        objs = [f for f in os.listdir(td) if "amdgcn" in f and "gfx950" in f]
        if len(objs) != 1:
            raise SystemExit(f"isa_same: {so}: expected one gfx950 code object, found {objs}")
        obj = os.path.join(td, objs[0])
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", obj], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--mcpu=gfx950", obj], check=True, capture_output=True,
                             text=True).stdout
    meta, blk = {}, {}
    for line in notes.splitlines() + ["  - "]:      # one "  - " block per kernel (a block's last .name is the kernel's, behind its arguments')
        if line.startswith("  - "):
            if "name" in blk:
                meta[blk.pop("name")] = blk
            blk = {}
        m = re.search(r"\.(name|%s):\s+(\S+)" % "|".join(META), line)
        if m:
            blk[m.group(1)] = m.group(2)
    kernels = set(meta)
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
    for ins in out.values():          # "s_nop 0" behind the last instruction: the assembler's padding behind a kernel that shares its section
        while ins and ins[-1] == "s_nop 0":      # with the next one (a non-template kernel; a template's section is padded by the linker)
            ins.pop()
    return out, meta


def demangle(names):
    """{symbol: demangled name}.  A c++filt that does not know the type code DF16_ (_Float16) leaves such names mangled: it is given
    the older code Dh (printed "half") and the name is put right afterwards, as tests/test_f16_cpu.py does."""
    names = list(names)
    dem = subprocess.run(["c++filt"] + [n.replace("DF16_", "Dh") for n in names], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dem) == len(names)
    return {n: re.sub(r"\bhalf\b", "_Float16", d) if "DF16_" in n else d for n, d in zip(names, dem)}


def read_map(path, dem_a, dem_b):
    """{symbol of the first library: symbol of the second} of the renamed kernels"""
    def one(frag, dem, which):
        hit = [n for n, d in dem.items() if ("fspann::" + frag + "(") in d]
        if len(hit) != 1:
            raise SystemExit(f"isa_same: {path}: '{frag}' matches {len(hit)} kernels of the {which} library, not one")
        return hit[0]
    ren = {}
    for line in open(path):
        if line.strip():
            old, new = line.rstrip("\n").split("\t")
            ren[one(old, dem_a, "first")] = one(new, dem_b, "second")
    return ren


def main(argv):
    verbose = "-v" in argv
    args = [a for a in argv if a != "-v"]
    mapfile = None
    if "--map" in args:
        at = args.index("--map")
        mapfile = args[at + 1]
        del args[at:at + 2]
    if len(args) != 2:
        raise SystemExit(__doc__)
    (a, ma), (b, mb) = kernel_isa(args[0]), kernel_isa(args[1])
    dem = demangle(set(a) | set(b))
    ren = read_map(mapfile, {n: dem[n] for n in a}, {n: dem[n] for n in b}) if mapfile else {}
    same, equiv, differ, missing = [], [], [], []
    for name, ins in sorted(a.items()):
        other = ren.get(name, name)
        if other not in b:
            missing.append(name)
        elif b[other] == ins:
            same.append(name)
        elif (len(b[other]) == len(ins) and collections.Counter(i.split()[0] for i in b[other]) == collections.Counter(i.split()[0] for i in ins)
              and ma[name] == mb[other]):
            equiv.append(name)
        else:
            differ.append(name)
    for n in equiv:
        x, y = a[n], b[ren.get(n, n)]
        lines = [(i, p, q) for i, (p, q) in enumerate(zip(x, y)) if p != q]
        print(f"EQUIVALENT  {dem[n]}: {len(x)} instructions, the same mnemonics and registers ({', '.join(f'{k} {v}' for k, v in ma[n].items())}), "
              f"{len(lines)} lines differ:")
        for i, p, q in lines:
            print(f"    #{i}: {p}  |  {q}")
    if verbose or differ or missing:
        for n in differ:
            x, y = a[n], b[ren.get(n, n)]
            at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            print(f"DIFFERS  {dem.get(n, n)}: {len(x)} vs {len(y)} instructions, first difference at #{at}: "
                  f"{x[at] if at < len(x) else '<end>'}  |  {y[at] if at < len(y) else '<end>'}")
        for n in missing:
            print(f"MISSING  {dem.get(n, n)}")
    ninstr = sum(len(a[n]) for n in same)
    print(f"isa_same: {len(a)} kernels in the first library: {len(same)} identical ({ninstr} instructions), {len(equiv)} equivalent, {len(differ)} differ, "
          f"{len(missing)} missing, {len(ren)} renamed; {len(set(b) - set(a) - set(ren.values()))} kernels only in the second")
    return 0 if not differ and not missing else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
