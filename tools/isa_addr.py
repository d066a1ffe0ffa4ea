"""How one kernel addresses global memory: its global loads and stores by address form — a 64-bit VGPR pair (`v[a:b], off`) or a scalar
base with one 32-bit VGPR offset (`v1, s[a:b]`) — and the 64-bit VALU arithmetic that builds the pairs, from an assembly file built with
the production flags plus `-S --cuda-device-only`.  The companion of tools/isa_mix.py (whose kernel lookup and cycle weights it reuses)
and tools/isa_lines.py; STATIC counts, every instruction once.
    python tools/isa_addr.py <file.s> <kernel-name-substring> [more substrings ...]
"""
import collections
import re
import sys

import isa_lines
import isa_mix

OPS64 = ("v_lshl_add_u64", "v_mov_b64", "v_lshlrev_b64", "v_addc_co_u32", "v_mad_u64_u32", "v_readlane_b32", "v_writelane_b32")


def count(asm, name, cyc):
    sym, body = isa_mix.kernel_body(asm, name)
    hist = collections.Counter()
    mem = collections.Counter()
    cycles = 0.0
    for l in body.split("\n"):
        l = l.strip()
        if not l or l.startswith(";") or l.startswith(".") or l.endswith(":"):
            continue
        op = l.split()[0]
        hist[re.sub(r"_(e32|e64)$", "", op)] += 1
        if op.startswith("v_"):
            cycles += isa_mix.klass(op, cyc)[0]
        m = re.match(r"global_(load|store|atomic)\w*\s+(.*)", l)
        if m:
            # the address operand is a VGPR pair in the 64-bit form and a single VGPR in front of an SGPR pair in the scalar-base form
            kind = m.group(1)
            ops = [o.strip() for o in m.group(2).split(",")]
            addr = ops[1] if kind == "load" or (kind == "atomic" and "sc0" in l and len(ops) > 3) else ops[0]
            mem[(kind, "vgpr pair" if addr.startswith("v[") else "scalar base")] += 1
    out = {"kernel": sym, "valu": sum(v for k, v in hist.items() if k.startswith("v_")), "valu_cycles": round(cycles),
           "salu": sum(v for k, v in hist.items() if k.startswith("s_"))}
    out.update(isa_lines.resources(asm, sym))
    for k in ("load", "store", "atomic"):
        out["global_%s vgpr pair / scalar base" % k] = "%d / %d" % (mem[(k, "vgpr pair")], mem[(k, "scalar base")])
    for op in OPS64:
        out[op] = hist[op]
    return out


def main():
    asm = open(sys.argv[1]).read()
    cyc = isa_mix.microbench(isa_mix.os.path.join(isa_mix.ROOT, "profiles", "r15_valu_peak_microbench.txt"))
    for name in sys.argv[2:]:
        r = count(asm, name, cyc)
        print(r.pop("kernel"))
        for k, v in r.items():
            print("  %-40s %s" % (k, v))


if __name__ == "__main__":
    main()
