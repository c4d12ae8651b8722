#!/usr/bin/env python3
"""Static instruction counts inside the loops of one kernel of a gfx950 assembly listing
(hipcc -S --cuda-device-only): the tables of DESIGN.md section 9, rounds 7-10.

    tools/loop_counts.py listing.s <substring of the kernel's mangled name> [min VALU, default 500]

A loop is a backward branch and its target label; the loops with at least `min VALU` vector
instructions are printed outermost first (in dcm_mpc_cold_kernel: the fp32 pass loop, then the fp64
pass loop, then the refinement).  VALU = every v_* but v_readlane / v_readfirstlane."""
import re
import sys


def kernel_lines(path, pat):
    out, on = [], False
    for ln in open(path):
        s = ln.strip()
        if not on:
            m = re.match(r"^(\S+):", s)
            if m and pat in m.group(1) and not s.startswith("."):
                on = True
            continue
        if s.startswith(".Lfunc_end"):
            break
        out.append(s)
    return out


def classify(ins):
    """ins: instruction lines.  Returns the counts of the table."""
    c = dict.fromkeys(("VALU", "mov_b32 reg", "mov_b32 const", "mov_b32 sgpr", "mov_b64 reg", "mov_b64 const",
                       "cndmask", "int addr/mask", "v_cmp", "saveexec", "SALU", "v_rcp", "ds_bpermute", "ds_read",
                       "v_cvt", "v_pk"), 0)
    for s in ins:
        op, _, rest = s.partition(" ")
        args = [a.strip() for a in rest.split(",")]
        if op.startswith("v_") and not op.startswith(("v_readlane", "v_readfirstlane")):
            c["VALU"] += 1
        if op.startswith("v_mov_b32") or op.startswith("v_mov_b64"):
            w = "mov_b32" if "b32" in op else "mov_b64"
            src = args[1] if len(args) > 1 else ""
            if "dpp" in s or "quad_perm" in s or "row_" in s or "wave_" in s:
                pass   # a lane shuffle, not a copy
            elif src.startswith("v"):
                c[w + " reg"] += 1
            elif src.startswith("s") and w == "mov_b32":
                c["mov_b32 sgpr"] += 1
            else:   # (a 64-bit move from an SGPR pair counts with the constants)
                c[w + " const"] += 1
        elif op.startswith("v_cndmask"):
            c["cndmask"] += 1
        elif re.match(r"v_(min|max)_[iu]32|v_lshl|v_lshr|v_ashr|v_add_u32|v_sub_u32|v_and_b32|v_or_b32|v_bfe|"
                      r"v_mul_u32_u24|v_mad_u32_u24|v_lshl_add|v_add_lshl|v_and_or|v_or3|v_xor|v_not|v_bcnt|v_ffb|"
                      r"v_subrev_u32|v_add3|v_lshl_or|v_mbcnt", op):
            c["int addr/mask"] += 1
        elif op.startswith("v_cmp"):
            c["v_cmp"] += 1
        elif op.startswith("v_rcp"):
            c["v_rcp"] += 1
        elif op.startswith("v_cvt"):
            c["v_cvt"] += 1
        elif op.startswith("v_pk_"):
            c["v_pk"] += 1
        elif op.startswith("ds_bpermute"):
            c["ds_bpermute"] += 1
        elif op.startswith("ds_read"):
            c["ds_read"] += 1
        if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_barrier")):
            c["SALU"] += 1
        if "saveexec" in op:
            c["saveexec"] += 1
    return c


def main():
    path, pat = sys.argv[1], sys.argv[2]
    floor = int(sys.argv[3]) if len(sys.argv) > 3 else 500
    lines = kernel_lines(path, pat)
    if not lines:
        sys.exit(f"no kernel matching {pat!r} in {path}")
    label = {}
    for i, s in enumerate(lines):
        m = re.match(r"^(\.LBB\S+):", s)
        if m:
            label[m.group(1)] = i
    loops = []
    for i, s in enumerate(lines):
        m = re.match(r"^s_c?branch\S*\s+(\.LBB\S+)", s)
        if m and m.group(1) in label and label[m.group(1)] < i:
            loops.append((label[m.group(1)], i, m.group(1)))
    # merge back edges to one header
    by_head = {}
    for a, b, name in loops:
        by_head[name] = (a, max(b, by_head.get(name, (a, b))[1]))
    isins = lambda s: s and not s.endswith(":") and not s.startswith((".", ";", "//"))
    whole = classify([s for s in lines if isins(s)])
    print(f"kernel: VALU {whole['VALU']}")
    for name, (a, b) in sorted(by_head.items(), key=lambda kv: kv[1]):
        c = classify([s for s in lines[a:b + 1] if isins(s)])
        if c["VALU"] >= floor:
            print(f"loop {name} (lines {a}-{b}): " + ", ".join(f"{k} {v}" for k, v in c.items()))


if __name__ == "__main__":
    main()
