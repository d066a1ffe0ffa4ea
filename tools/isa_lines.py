"""Where one kernel's instructions come from, by source line: a histogram over the `.loc` lines of an assembly file built with
line tables (the production flags plus `-gline-tables-only -S --cuda-device-only`).  The companion of tools/isa_mix.py, whose kernel
lookup and per-opcode issue cycles it reuses: a line's VALU weight is given in issue cycles as well as in instructions.
The counts are STATIC — every instruction once, an inlined function once per copy, attributed to the innermost line the compiler
names; an instruction in front of the kernel's first `.loc` counts under `?:0`.  The tool reads what the compiler wrote, nothing else.
    python tools/isa_lines.py <file.s> <kernel-name-substring> [--top N] [--microbench file]
Columns: VALU instructions, their issue cycles, s_nop, SALU (every other s_ instruction), LDS (ds_), vector memory (global_ / flat_ /
buffer_ / scratch_), 64-bit shifts (part of VALU), cross-lane (ds_bpermute / ds_permute / ds_swizzle, DPP, v_readlane / v_writelane /
v_readfirstlane / v_permlane: part of VALU or LDS).  Lines are ordered by VALU + s_nop; --top 0 prints them all.
"""
import argparse
import collections
import os
import re

import isa_mix

COLS = ("valu", "cycles", "s_nop", "salu", "lds", "vmem", "shift64", "xlane")
SHIFT64 = ("v_lshlrev_b64", "v_lshrrev_b64", "v_ashrrev_i64")


def kinds(op):
    """the columns one instruction counts in (cycles apart)"""
    base = re.sub(r"_(e32|e64|sdwa|dpp)$", "", op)
    out = []
    if op == "s_nop":
        out.append("s_nop")
    elif op.startswith("s_"):
        out.append("salu")
    elif op.startswith("v_"):
        out.append("valu")
    elif op.startswith("ds_"):
        out.append("lds")
    elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        out.append("vmem")
    if base in SHIFT64:
        out.append("shift64")
    if (op.endswith("_dpp") or base.startswith(("ds_bpermute", "ds_permute", "ds_swizzle", "v_readlane", "v_writelane", "v_readfirstlane",
                                                 "v_permlane"))):
        out.append("xlane")
    return out


def resources(asm, sym):
    """codeLenInByte, VGPRs and scratch of the kernel, from the comment block the compiler writes behind its code"""
    at = asm.find("\n%s:" % sym)
    out = {}
    for key, pat in (("codeLenInByte", r"; codeLenInByte = (\d+)"), ("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)"),
                     ("sgprs", r"; NumSgprs: (\d+)"), ("scratch_bytes", r"; ScratchSize: (\d+)"), ("lds_bytes", r"; LDSByteSize: (\d+)"),
                     ("occupancy", r"; Occupancy: (\d+)")):
        m = re.compile(pat).search(asm, at)
        out[key] = int(m.group(1)) if m else None
    return out


def histogram(asm, body, cyc):
    files = {}
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', asm, re.M):
        files[int(m.group(1))] = os.path.basename(m.group(3))
    rows = collections.defaultdict(lambda: collections.Counter())
    cur = ("?", 0)
    for l in body.split("\n"):
        l = l.strip()
        if l.startswith(".loc"):
            p = l.split()
            cur = (files.get(int(p[1]), "file%s" % p[1]), int(p[2]))
            continue
        if not l or l.startswith(";") or l.startswith(".") or l.endswith(":"):
            continue
        op = l.split()[0]
        for k in kinds(op):
            rows[cur][k] += 1
        if op.startswith("v_"):
            rows[cur]["cycles"] += isa_mix.klass(op, cyc)[0]
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--top", type=int, default=80, help="lines to print (0: all)")
    ap.add_argument("--microbench", default=os.path.join(isa_mix.ROOT, "profiles", "r15_valu_peak_microbench.txt"))
    a = ap.parse_args()
    asm = open(a.asm).read()
    cyc = isa_mix.microbench(a.microbench)
    sym, body = isa_mix.kernel_body(asm, a.kernel)
    rows = histogram(asm, body, cyc)
    if len(rows) <= 1:
        raise SystemExit("no .loc lines in %s: build the assembly with -gline-tables-only" % sym)
    total = collections.Counter()
    for r in rows.values():
        total.update(r)
    print("kernel %s" % sym)
    print("  ".join("%s %s" % (k, v) for k, v in resources(asm, sym).items()))
    print("instructions %d" % (total["valu"] + total["s_nop"] + total["salu"] + total["lds"] + total["vmem"]))
    head = "%-26s" % "file:line" + "".join("%9s" % c for c in COLS)
    print(head)

    def fmt(name, r):
        return "%-26s" % name + "".join(("%9.0f" if c == "cycles" else "%9d") % r[c] for c in COLS)

    print(fmt("TOTAL", total))
    order = sorted(rows.items(), key=lambda kv: (-(kv[1]["valu"] + kv[1]["s_nop"]), kv[0]))
    shown = order if a.top <= 0 else order[:a.top]
    for (f, ln), r in shown:
        print(fmt("%s:%d" % (f, ln), r))
    if len(shown) < len(order):
        rest = collections.Counter()
        for _, r in order[len(shown):]:
            rest.update(r)
        print(fmt("(%d more lines)" % (len(order) - len(shown)), rest))
    by_file = collections.defaultdict(collections.Counter)
    for (f, _), r in rows.items():
        by_file[f].update(r)
    print()
    for f, r in sorted(by_file.items(), key=lambda kv: -kv[1]["valu"]):
        print(fmt(f + ":*", r))


if __name__ == "__main__":
    main()
