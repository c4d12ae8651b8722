"""Refactoring check per kernel: whether every kernel csrc/<src>.hip had at <rev> still compiles to the
same gfx950 assembly, when the change ADDS kernels to the file (tools/isa_same.sh compares the whole
listing and so reports the additions).
  python tools/isa_same_kernels.py <src> [<rev>]      (rev defaults to HEAD~1)
Compiles both with the Makefile's flags for build/<src>.o, splits the listings at the function symbols,
drops comments and renumbers the block labels (.LBB<function>_<block>: the function index shifts when
kernels are added before one), and compares function by function.  Compiles and compares only; nothing
runs on a GPU."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "bipedal-locomotion-framework_amd"


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
        ln = re.sub(r"\s*;.*$", "", ln)
        if ln.strip():
            cur.append(re.sub(r"\.LBB\d+_", ".LBBx_", re.sub(r"\.Ltmp\d+", ".Ltmp", ln)))
    return out


def main():
    src, rev = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "HEAD~1")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(f"git -C {ROOT} archive {rev} {PKG}/csrc include | tar -x -C {tmp}", shell=True)
        cc = subprocess.check_output(f"make -C {ROOT}/{PKG} --no-print-directory -n -B build/{src}.o | "
                                     f"sed -n 's| -c csrc/{src}\\.hip.*||p'", shell=True, text=True).strip()
        asm = lambda d: subprocess.check_output(f"cd {d}/{PKG} && {cc} --cuda-device-only -S csrc/{src}.hip -o -",
                                                shell=True, text=True, stderr=subprocess.DEVNULL)
        with cf.ThreadPoolExecutor(2) as ex:
            fo, fn = ex.submit(asm, tmp), ex.submit(asm, ROOT)
            old, new = functions(fo.result()), functions(fn.result())
    bad = 0
    for k, v in old.items():
        if k not in new:
            print("missing:", k)
            bad += 1
        elif new[k] != v:
            first = next(((a, b) for a, b in zip(v, new[k]) if a != b), (len(v), len(new[k])))
            print("differs:", k, first)
            bad += 1
    print(f"{len(old)} functions at {rev}, {len(new)} now ({len(new) - len(old) + sum(k not in new for k in old)} added), "
          f"{bad} differ" + ("" if bad else ": identical"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
