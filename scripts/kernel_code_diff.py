#!/usr/bin/env python3
"""Compare two `llvm-objdump -d` listings of gfx950 code objects function by function: the instruction sequences with
the address / encoding column dropped and the literal of a pc-relative symbol reference (the s_add_u32 / s_addc_u32
after an s_getpc_b64) masked.  Functions are paired by their last name component, so a kernel that moved to another
namespace still pairs.  Exit status 1 if a paired function differs or a function has no partner.
usage: python scripts/kernel_code_diff.py <parent.dis> <new.dis> [name substring]"""
import difflib
import re
import sys


def last_component(sym):
    """`_ZN3lrl4flat15env_step_kernelILb0EEEv...` -> `env_step_kernel` (an unmangled or unnested name: itself)"""
    rest, name = sym[3:] if sym.startswith("_ZN") else "", sym
    while (m := re.match(r"(\d+)", rest)):
        n = int(m.group(1))
        name, rest = rest[m.end():m.end() + n], rest[m.end() + n:]
    return name


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = out.setdefault(last_component(m.group(1)), [])
        elif cur is not None and line.startswith("\t"):
            ins = line.split("//")[0].strip()
            if ins == "...":  # (objdump's elision of trailing zero padding)
                continue
            if len(cur) and any("s_getpc_b64" in p for p in cur[-2:]) and re.match(r"s_addc?_u32", ins):
                ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "<rel>", ins)
            cur.append(ins)
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
want = sys.argv[3] if len(sys.argv) > 3 else ""
bad = 0
for name in sorted(set(a) | set(b)):
    if want not in name:
        continue
    if name not in a or name not in b:
        print(f"{name}: only in {'parent' if name in a else 'new'}")
        bad = 1
        continue
    sm = difflib.SequenceMatcher(None, a[name], b[name], autojunk=False)
    diff = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
    print(f"{name}: {len(a[name])} vs {len(b[name])} instructions, {diff} differ")
    bad |= diff != 0
sys.exit(bad)
