#!/bin/bash
# Refactoring check: whether a change to one kernel source left its device code untouched.
#   tools/isa_same.sh <src> [<rev>]
# Compiles csrc/<src>.hip of <rev> (default HEAD~1) and of the working tree to gfx950 assembly with
# the Makefile's flags for build/<src>.o, drops the lines naming the __hip_cuid_<hash> symbol (a
# hash of the source text) and compares.  Compiles and compares only; nothing runs on a GPU.
set -euo pipefail
src=$1; rev=${2:-HEAD~1}
root=$(cd "$(dirname "$0")/.." && pwd); pkg=bipedal-locomotion-framework_amd
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old"
git -C "$root" archive "$rev" $pkg/csrc include | tar -x -C "$tmp/old"
# the object's compile line as make would run it, up to the "-c <source> -o <object>"
cc=$(make -C "$root/$pkg" --no-print-directory -n -B build/$src.o | sed -n "s| -c csrc/$src\.hip.*||p")
asm() { (cd "$1/$pkg" && eval "$cc --cuda-device-only -S csrc/$src.hip -o -") | grep -v __hip_cuid_ > "$2"; }
asm "$tmp/old" "$tmp/old.s" & asm "$root" "$tmp/new.s"; wait $!
if cmp -s "$tmp/old.s" "$tmp/new.s"; then echo identical
else diff "$tmp/old.s" "$tmp/new.s" | head -40; exit 1; fi
