"""Refactoring check per kernel: whether every kernel csrc/<src>.hip had at <rev> still compiles to the
same gfx950 assembly, when the change ADDS or RENAMES kernels in the file (tools/isa_same.sh compares
the whole listing and so reports the additions).
  python tools/isa_same_kernels.py <src> [<rev>] [--rename OLD=NEW]... [--allow-kernarg-offsets]
(rev defaults to HEAD~1).  Compiles both with the Makefile's flags for build/<src>.o, splits the listings
at the function symbols, drops comments and renumbers the block labels (.LBB<function>_<block>: the
function index shifts when kernels are added before one), and compares function by function.
--rename is a regex substitution on the old listing's mangled names before pairing, for a kernel whose
name or template arguments changed.  A function whose only differences are the offset immediates of
scalar loads from the kernarg segment (a kernel argument moved; same opcode, same registers, same line
count) is counted on its own and passes only with --allow-kernarg-offsets.  Compiles and compares only;
nothing runs on a GPU."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "bipedal-locomotion-framework_amd"

# A scalar load through s[0:1]: these code objects enable the kernarg segment pointer as their only user
# SGPR pair, so that is where it arrives.  (A load through a copy of the pointer is not recognised and
# counts as a plain difference.)
KERNARG_LOAD = re.compile(r"^(\s*s_load_dword(?:x\d+)?\s+s(?:\d+|\[\d+:\d+\]),\s*s\[0:1\],\s*)(0x[0-9a-f]+|\d+)\s*$")


def functions(text):
    out, cur, name = {}, None, None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name], cur = cur, None
            continue
        # (the kernel descriptor's directives inside the function's range carry its own name)
        ln = re.sub(r"\s*;.*$", "", ln).replace(name, "<self>")
        if ln.strip():
            cur.append(re.sub(r"\.LBB\d+_", ".LBBx_", re.sub(r"\.Ltmp\d+", ".Ltmp", ln)))
    return out


def classify(old, new):
    """One function's two bodies (lists of lines from functions()): the verdict and the differing line pairs."""
    if old == new:
        return "identical", []
    diffs = [(a, b) for a, b in zip(old, new) if a != b]
    if len(old) != len(new):
        return "differs", diffs or [(len(old), len(new))]
    for a, b in diffs:
        ma, mb = KERNARG_LOAD.match(a), KERNARG_LOAD.match(b)
        if not (ma and mb and ma.group(1) == mb.group(1)):
            return "differs", diffs
    return "kernarg-offset", diffs


def compare(old_text, new_text, renames=()):
    """Pairs the functions of two listings by mangled name, the old names first rewritten by `renames`
    ((regex, replacement) pairs), and classifies each pair.
    Returns ({old name: (verdict, differing line pairs)}, functions in the old listing, in the new one);
    a verdict is identical, kernarg-offset, differs or missing."""
    old, new = functions(old_text), functions(new_text)
    res = {}
    for k, v in old.items():
        to = k
        for pat, rep in renames:
            to = re.sub(pat, rep, to)
        res[k] = classify(v, new[to]) if to in new else ("missing", [])
    return res, len(old), len(new)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--allow-kernarg-offsets", action="store_true")
    a = ap.parse_args()
    src, rev = a.src, a.rev
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(f"git -C {ROOT} archive {rev} {PKG}/csrc include | tar -x -C {tmp}", shell=True)
        cc = subprocess.check_output(f"make -C {ROOT}/{PKG} --no-print-directory -n -B build/{src}.o | "
                                     f"sed -n 's| -c csrc/{src}\\.hip.*||p'", shell=True, text=True).strip()
        asm = lambda d: subprocess.check_output(f"cd {d}/{PKG} && {cc} --cuda-device-only -S csrc/{src}.hip -o -",
                                                shell=True, text=True, stderr=subprocess.DEVNULL)
        with cf.ThreadPoolExecutor(2) as ex:
            fo, fn = ex.submit(asm, tmp), ex.submit(asm, ROOT)
            res, nold, nnew = compare(fo.result(), fn.result(), renames)
    count = {v: sum(r[0] == v for r in res.values()) for v in ("identical", "kernarg-offset", "differs", "missing")}
    for k, (verdict, diffs) in res.items():
        if verdict == "missing":
            print("missing:", k)
        elif verdict == "differs":
            print("differs:", k, diffs[0])
        elif verdict == "kernarg-offset":
            print("kernarg offsets only:", k, *diffs)
    bad = count["differs"] + count["missing"]
    paired = nold - count["missing"]
    print(f"{nold} functions at {rev}, {nnew} now ({nnew - paired} added): {paired} paired, {count['missing']} missing, "
          f"{count['differs']} differ, {count['kernarg-offset']} differ only in kernarg load offsets"
          + ("" if bad or count["kernarg-offset"] else ": identical"))
    sys.exit(1 if bad or (count["kernarg-offset"] and not a.allow_kernarg_offsets) else 0)


if __name__ == "__main__":
    main()
