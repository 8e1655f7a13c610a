#!/bin/bash
# gfx950 disassembly of every code object of a built library: scripts/disasm.sh <lib.so> <out.s>
# (one offload bundle per translation unit, extracted as check_code_object.py does).  The output holds no addresses --
# no leading ones, no trailing `// <address>: <encoding>` comments --, so `diff` of two builds shows only changed code.
set -e
L=/opt/rocm/lib/llvm/bin
D=$(cd "$(dirname "$0")" && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
python3 -c 'import sys; sys.path.insert(0, sys.argv[1]); import check_code_object as c
print("\n".join(c.extract_code_objects(sys.argv[2], sys.argv[3])))' "$D" "$1" "$T" > "$T/cos"
: > "$2"
k=0
while read -r co; do
  echo "// code object $k" >> "$2"
  $L/llvm-objdump -d --no-show-raw-insn --no-leading-addr "$co" |
    sed -E '/:[[:space:]]+file format /d; s#[[:space:]]*// [0-9A-F]+:.*$##' | c++filt >> "$2"
  k=$((k + 1))
done < "$T/cos"
