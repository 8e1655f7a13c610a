#!/usr/bin/env python3
"""Compare two code-object tables (scripts/check_code_object.py --json) kernel by kernel.

    python3 scripts/check_code_object.py --quiet --so <parent lib> --json parent.json
    python3 scripts/check_code_object.py --quiet --so <branch lib> --json branch.json
    python3 scripts/code_object_diff.py parent.json branch.json > profiles/<name>_code_object_diff.txt

A kernel present in both tables must keep its VGPR and AGPR count, static LDS bytes, scratch and spills (exit code 1
otherwise); SGPR counts may move and are listed.  A moved SGPR-SPILL count is listed apart: spilled scalars travel
through v_writelane / v_readlane, and where those land inside a loop the kernel's steady state has changed although its
VGPR count has not -- compare the loop bodies (scripts/disasm.sh on both builds) before calling such a build equal.
Kernels only one side has are listed.  No GPU needed: this is how a
never-taken path that costs a hot kernel registers is caught before anything runs.
"""
import json
import sys

PINNED = ("vgpr", "agpr", "lds_static", "scratch", "vgpr_spills")


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a = {k["kernel"]: k for k in json.load(open(sys.argv[1]))["kernels"]}
    b = {k["kernel"]: k for k in json.load(open(sys.argv[2]))["kernels"]}
    both = sorted(set(a) & set(b))
    bad, moved = [], []
    for n in both:
        d = [(f, a[n].get(f), b[n].get(f)) for f in PINNED if a[n].get(f) != b[n].get(f)]
        if d:
            bad.append((n, d))
        for f in ("sgpr", "sgpr_spills"):
            if a[n].get(f) != b[n].get(f):
                moved.append((n, f, a[n].get(f), b[n].get(f)))
    print("kernels: %d before, %d after, %d in both" % (len(a), len(b), len(both)))
    for n in sorted(set(a) - set(b)):
        print("removed: %s" % n)
    for n in sorted(set(b) - set(a)):
        k = b[n]
        print("new:     %s  vgpr %d sgpr %d lds %d scratch %d" % (n, k["vgpr"], k["sgpr"], k["lds_static"], k["scratch"]))
    print("VGPR / AGPR / LDS / scratch / vector spills changed in %d of %d kernels" % (len(bad), len(both)))
    for n, d in bad:
        print("  CHANGED %s: %s" % (n, ", ".join("%s %s -> %s" % x for x in d)))
    plain = [m for m in moved if m[1] == "sgpr"]
    spills = [m for m in moved if m[1] == "sgpr_spills"]
    print("SGPR count moved in %d kernels (allowed)" % len(plain))
    for n, f, x, y in plain:
        print("  %s: %s %s -> %s" % (n, f, x, y))
    print("SGPR spills moved in %d kernels (lane moves: check whether they sit in loops, scripts/disasm.sh)" % len(spills))
    for n, f, x, y in spills:
        print("  %s: %s %s -> %s" % (n, f, x, y))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
