#!/usr/bin/env python3
"""Instruction budget of a kernel's hot loop from a device-only assembly dump (hipcc --offload-device-only -S).

    python tools/isa_budget.py file.s <kernel-symbol-substring> [--min-block N] [--products P]

The loop is the innermost loop of the kernel with the most instructions (the compiler's own `Loop Header` comments).  Its
basic blocks are split in two: the LONG straight-line blocks (at least N instructions, default 64, no call) -- in a formula kernel
these are the field products and the linear operations between them, which every iteration executes -- and the REST of the loop
(the exceptional-case filter, its out-of-line branches, loop control), of which an iteration runs only a path.  Where the compiler
cuts the blocks differs from build to build, so two builds are compared on the WHOLE-LOOP column.  The table gives the opcode
classes that matter on the integer VALU:

    multiply-add            v_mad_u64_u32 / v_mad_i64_i32
    zero-shift 64-bit add   v_lshl_add_u64 x, y, 0, z: a plain 64-bit add (a column sum joined to the previous column's carry)
    64-bit shift            v_lshrrev_b64 / v_lshlrev_b64 / v_ashrrev_i64
    mask                    v_and_b32
    mul_lo                  v_mul_lo_u32
    other VALU              everything else that starts with v_
    VMEM                    global / flat / buffer / scratch loads and stores
    SALU                    s_* except s_nop and s_waitcnt (listed apart: they issue, but not on an ALU)

With --products P the zero-shift adds are also given per field product.  A developer tool: nothing runs it automatically."""
import argparse
import re
from collections import Counter

CLASSES = ["multiply-add", "zero-shift 64-bit add", "64-bit shift", "mask", "mul_lo", "other VALU", "VMEM", "SALU", "s_nop", "s_waitcnt", "other"]


def classify(line):
    op = line.split()[0]
    if op.startswith(("v_mad_u64_u32", "v_mad_i64_i32")):
        return "multiply-add"
    if op.startswith("v_lshl_add_u64"):
        args = [a.strip() for a in line.split(None, 1)[1].split(",")]
        # v_lshl_add_u64 vdst(pair), src0(pair), shift, src2(pair)
        return "zero-shift 64-bit add" if len(args) == 4 and args[2] == "0" else "other VALU"
    if op.startswith(("v_lshrrev_b64", "v_lshlrev_b64", "v_ashrrev_i64")):
        return "64-bit shift"
    if op.startswith("v_and_b32"):
        return "mask"
    if op.startswith("v_mul_lo_u32"):
        return "mul_lo"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def function_lines(path, needle):
    """(symbol, the lines of its body, the register / scratch figures the compiler prints after it)"""
    out, meta, on, name = [], {}, 0, None
    with open(path) as f:
        for l in f:
            if on == 0:
                m = re.match(r"^([A-Za-z_][\w.$]*):", l)
                if m and needle in m.group(1) and not m.group(1).startswith(".L"):
                    on, name = 1, m.group(1)
            elif on == 1:
                if l.startswith(".Lfunc_end"):
                    on = 2
                else:
                    out.append(l.rstrip("\n"))
            else:
                m = re.match(r"\s*; (NumVgprs|ScratchSize|Occupancy): (\d+)", l)
                if m:
                    meta[m.group(1)] = int(m.group(2))
                elif re.match(r"^[A-Za-z_][\w.$]*:", l):
                    break
    if name is None:
        raise SystemExit("no function whose symbol contains %r in %s" % (needle, path))
    return name, out, meta


def is_inst(s):
    return bool(s) and not s.startswith((";", ".")) and not s.endswith(":") and not re.match(r"^[\w.$]+:\s*(;.*)?$", s)


def blocks_of_loop(lines):
    """basic blocks (lists of instruction lines) of the innermost loop with the most instructions"""
    # every label line carries `Header=BBx_y` (a member) or `Loop Header` (the header itself); the code before the first label after
    # a header belongs to the header
    owner, cur = [], None
    for l in lines:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):\s*;(.*)$", s)
        if m:
            lab, com = m.group(1)[2:], m.group(2)
            h = re.search(r"Header=(BB\d+_\d+)", com)
            if "Inner Loop Header" in com:
                cur = lab
            elif h and "Depth" in com:
                cur = h.group(1)
            elif "Loop Header" in com:
                cur = None            # an outer loop's header: its own code is not part of an innermost loop
            else:
                cur = None
        owner.append(cur)
    sizes = Counter(o for o, l in zip(owner, lines) if o and is_inst(l.strip()))
    if not sizes:
        raise SystemExit("no loop found")
    loop = sizes.most_common(1)[0][0]
    blocks, b = [], []
    for o, l in zip(owner, lines):
        s = l.strip()
        if o != loop:
            if b:
                blocks.append(b); b = []
            continue
        if re.match(r"^\.LBB\d+_\d+:", s) and b:
            blocks.append(b); b = []
        if is_inst(s):
            b.append(s)
            if s.startswith(("s_cbranch", "s_branch", "s_setpc")):
                blocks.append(b); b = []
    if b:
        blocks.append(b)
    return loop, blocks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--min-block", type=int, default=64)
    ap.add_argument("--products", type=int, default=0)
    a = ap.parse_args()
    name, lines, meta = function_lines(a.asm, a.symbol)
    loop, blocks = blocks_of_loop(lines)
    long_c, rest_c, nlong = Counter(), Counter(), 0
    for b in blocks:
        is_long = len(b) >= a.min_block and not any(s.startswith("s_swappc") for s in b)
        nlong += is_long
        (long_c if is_long else rest_c).update(classify(s) for s in b)
    print("kernel  %s" % name)
    print("loop    %s: %d basic blocks, %d of them long (>= %d instructions, no call)" % (loop, len(blocks), nlong, a.min_block))
    print("meta    " + ", ".join("%s %d" % kv for kv in sorted(meta.items())))
    print()
    print("| class | long blocks | rest of loop | whole loop |")
    print("|---|---:|---:|---:|")
    for c in CLASSES:
        if long_c[c] or rest_c[c]:
            print("| %s | %d | %d | %d |" % (c, long_c[c], rest_c[c], long_c[c] + rest_c[c]))
    valu = CLASSES[:6]
    vl, vr = sum(long_c[c] for c in valu), sum(rest_c[c] for c in valu)
    print("| **VALU total** | %d | %d | %d |" % (vl, vr, vl + vr))
    if a.products:
        print()
        print("zero-shift 64-bit adds per product (long blocks / %d): %.1f" % (a.products, long_c["zero-shift 64-bit add"] / a.products))


if __name__ == "__main__":
    main()
